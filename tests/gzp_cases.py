"""Plain-gzip inputs for the K-GUNZIP tests, all made here with zlib: the streams A - G of the issue (raw deflate streams and their
texts), gzip members and files around them with every optional header field, and the streams that are refused by name.  The BGZF side
and the hand-made blocks are gz_cases'."""
import random
import struct
import zlib

import gz_cases as gz

# pf_gunzip::Clause (csrc/pf_gunzip_core.hpp), numbered behind pf_inflate's
CLAUSES = ["reserved_flag", "header_past", "cut_block", "cut_trailer", "trailing", "block_too_large", "piece_limit"]
CLAUSE = dict(gz.CLAUSE, **{name: len(gz.CLAUSES) + i for i, name in enumerate(CLAUSES)})
PIECES = (64, 1024, 16384, 1 << 30)
HEADER = b"\x1f\x8b\x08\x00\0\0\0\0\x00\xff"


def raw(text: bytes, level: int = 6, mem: int = 8, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_at=()) -> bytes:
    """zlib's raw deflate stream; flush_at: (position, flush mode), ascending"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = b"", 0
    for pos, mode in flush_at:
        out += c.compress(text[at:pos]) + c.flush(mode)
        at = pos
    return out + c.compress(text[at:]) + c.flush()


def header(name=None, extra=None, comment=None, hcrc=False, text_flag=False) -> bytes:
    flg = (1 if text_flag else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def trailer(text: bytes) -> bytes:
    return struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def member(text: bytes, stream=None, head: bytes = HEADER) -> bytes:
    return head + (raw(text) if stream is None else stream) + trailer(text)


def text_a() -> bytes:
    return gz.fastq(2000, seed=7)


def text_c(repeat: bool = True) -> bytes:
    """200 random bytes, 32 200 bytes of ACGTN noise, the same 200 bytes, four times over: the random bytes can only be matched at
    distance 32 400 (zlib looks back 32 506 bytes at most), and more compressed bytes than several pieces lie between two copies.  repeat=False: other random bytes each
    time -- what the stream costs when nothing matches far back"""
    rnd = random.Random(23)
    fars = [bytes(rnd.randrange(256) for _ in range(200)) for _ in range(5)]
    noise = [bytes(rnd.choice(b"ACGTN") for _ in range(32200)) for _ in range(4)]
    return b"".join((fars[0] if repeat else fars[i]) + noise[i] for i in range(4)) + (fars[0] if repeat else fars[4])


def flushes(n: int, step: int = 5000):
    modes = [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]
    return [(p, modes[(p // step) % 2]) for p in range(step, n, step)]


_cache = {}


def streams():
    """{name: (raw deflate stream, text)}: A - F of the issue"""
    if _cache:
        return _cache
    a = text_a()
    s = {"A": (raw(a, 6, 8), a), "B": (raw(a, 6, 1), a)}
    c = text_c()
    s["C"] = (raw(c, 9, 4), c)   # (memLevel 4: blocks of 1 024 symbols, so that pieces lie between the copies)
    s["D_flush"] = (raw(a, 6, 8, flush_at=flushes(len(a))), a)
    s["D_block"] = (raw(a, 6, 8, flush_at=[(p, zlib.Z_BLOCK) for p in range(5000, len(a), 5000)]), a)
    s["E_stored"] = (raw(a, 0), a)
    s["E_fixed"] = (raw(a, 6, 8, zlib.Z_FIXED), a)
    for name, text in gz.texts():
        for setting, level, strategy in gz.SETTINGS:
            s["F_%s_%s" % (name, setting)] = (raw(text, level, 8, strategy), text)
    _cache.update(s)
    return _cache


def files():
    """{name: (file bytes, text)}: G of the issue -- several members, one of them empty, every optional header field"""
    a, b, c = gz.fastq(300, seed=1), gz.fastq(150, seed=2), gz.fastq(40, seed=3)
    return {
        "one_plain": (member(a), a),
        "name": (member(a, head=header(name=b"reads.fastq")), a),
        "extra_not_bc": (member(a, head=header(extra=b"XY\x03\x00abc")), a),
        "extra_04_no_bc": (member(a, head=b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0XY\x02\0\x00\x00"), a),
        "comment_hcrc_text": (member(a, head=header(comment=b"a comment", hcrc=True, text_flag=True)), a),
        "all_fields": (member(a, head=header(name=b"n", extra=b"AB\x01\x00z", comment=b"c", hcrc=True)), a),
        "two_members": (member(a) + member(b, head=header(name=b"lane2.fq")), a + b),
        "three_one_empty": (member(a) + member(b"") + member(c, raw(c, 1)), a + c),
        "empty_first": (member(b"") + member(b), b),
        "only_empty": (member(b""), b""),
    }


def stream_refusals():
    """{clause name: raw stream}: deflate streams the decoder refuses by that clause, at their first block (gz_cases' hand-made blocks)"""
    m = gz.stream_clause_members()
    return {name: m[name][18:-8] for name in ("btype3", "stored_len", "too_many_codes", "code_lengths", "repeat", "no_eob", "bad_code", "litlen_sym",
                                              "dist_sym", "dist_before")}


def sound_prefix():
    """(raw stream without a final block, ending at a byte boundary; its text): what a refused block is put behind"""
    text = gz.fastq(120, seed=4)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    return c.compress(text[:9000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[9000:]) + c.flush(zlib.Z_SYNC_FLUSH), text
