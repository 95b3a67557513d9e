"""What the tests of the one deflate decoder behind K-INFLATE and K-GUNZIP share: the members both drivers are run on, the streams at
the edges of the window in LDS, and the records tests/cpp/gz_decode_dump.cpp reads."""
import struct
import zlib

import gz_cases as gz
import gzp_cases as gp

_members = []


def members():
    """[(name, raw deflate payload, text)]: every text of gz_cases under every compressor setting that fits a BGZF member"""
    if not _members:
        for name, text in gz.texts():
            for setting, level, strategy in gz.SETTINGS:
                if gz.member_fits(text, level, strategy):
                    _members.append(("%s_%s" % (name, setting), gz.deflate(text, level, strategy), text))
    return _members


# Payload lengths on both sides of the first two refill points of a 1024-byte window that keeps 64 bytes: byte 1024 is the first one
# outside the first window, which then moves to [960, 1984).  A fixed-code literal below 144 is eight bits, so a text of n such bytes
# gives a payload of n + 2 bytes (three header bits, seven of the end-of-block code, padding).
WINDOW_EDGE_LENGTHS = (1022, 1023, 1024, 1025, 1026, 1982, 1983, 1984, 1985, 1986)


def window_edge_streams():
    """[(payload, text)]: fixed-code literal streams of exactly the WINDOW_EDGE_LENGTHS"""
    out = []
    for n in WINDOW_EDGE_LENGTHS:
        text = gz.fastq(30, seed=n)[: n - 2]
        payload = gz.fixed_literals(text)
        assert len(payload) == n and zlib.decompress(payload, -15) == text
        out.append((payload, text))
    return out


def dump_records(full: bool) -> bytes:
    """the records file of gz_decode_dump: 1 = a raw stream, 2 = its text (only its length and CRC matter where the stream is broken),
    4 = a refused stream behind a byte that is not looked at.  full: every stream of gz_cases and gzp_cases; otherwise the small ones"""
    recs = []
    for name, (stream, text) in gp.streams().items():
        if full or len(stream) <= 1200:
            recs += [(1, stream), (2, text)]
    few = gz.fastq(5, seed=3)
    recs += [(1, gz.fixed_literals(few[:300])), (2, few[:300]), (1, gz.dynamic_literals(few[:300])), (2, few[:300])]
    prefix, ptext = gp.sound_prefix()
    if full:
        recs += [(1, prefix), (2, ptext)]
    for name, m in gz.stream_clause_members().items():   # as K-INFLATE sees them: with the member's own ISIZE
        recs += [(1, m[18:-8]), (2, bytes(struct.unpack("<I", m[-4:])[0]))]
    recs += [(4, bytes([gp.CLAUSE[name]]) + bad) for name, bad in gp.stream_refusals().items()]
    return b"".join(struct.pack("<II", tag, len(b)) + b for tag, b in recs)
