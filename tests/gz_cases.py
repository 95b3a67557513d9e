"""Blocked-gzip inputs for the K-INFLATE tests, all made here: BGZF members around zlib's raw deflate streams (every kind of block the
compressor writes), members written bit by bit (fixed and dynamic blocks that no compressor emits, one per refusal), texts, and files
cut into members as `bgzip` cuts them."""
import random
import struct
import zlib

# pf_inflate::Clause (csrc/pf_inflate_core.hpp), in its order
CLAUSES = ["none", "magic", "not_blocked", "method", "flags", "short", "past_end", "isize", "btype3", "stored_len", "stored_past", "too_many_codes",
           "code_lengths", "repeat", "no_eob", "bad_code", "litlen_sym", "dist_sym", "dist_before", "out_beyond", "end", "length", "crc"]
CLAUSE = {name: i for i, name in enumerate(CLAUSES)}
CLAUSE_WORDS = {   # a word of each clause's text
    "magic": "magic 1f 8b", "not_blocked": "bgzip", "method": "method is not 8", "flags": "FEXTRA", "short": "shorter than its header and trailer",
    "past_end": "past the end of the file", "isize": "ISIZE is above 65536", "btype3": "type 3", "stored_len": "LEN and NLEN",
    "stored_past": "stored block runs past", "too_many_codes": "more than 286", "code_lengths": "over-subscribed or incomplete",
    "repeat": "repeat code", "no_eob": "end-of-block", "bad_code": "no code of", "litlen_sym": "286 or 287", "dist_sym": "30 or 31",
    "dist_before": "before the member's first byte", "out_beyond": "more bytes than ISIZE", "end": "does not end at the trailer",
    "length": "differs from ISIZE", "crc": "CRC-32 mismatch"}
STREAM_CLAUSES = CLAUSES[CLAUSE["btype3"]:]

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZIP_CUT = 65536 - 256   # bytes of text `bgzip` puts into a member

SETTINGS = [("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("level1", 1, zlib.Z_DEFAULT_STRATEGY),
            ("level6", 6, zlib.Z_DEFAULT_STRATEGY), ("level9", 9, zlib.Z_DEFAULT_STRATEGY), ("huffman", 6, zlib.Z_HUFFMAN_ONLY),
            ("rle", 6, zlib.Z_RLE)]


def wrap(raw: bytes, text_crc: int, isize: int, extra_before: bytes = b"") -> bytes:
    """a BGZF member around the deflate stream `raw`; extra_before: subfields in front of BC"""
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(raw) + 8 - 1
    assert bsize <= 0xFFFF, bsize
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\0" + struct.pack("<H", bsize) + raw +
            struct.pack("<II", text_crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def deflate(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_at=()) -> bytes:
    """zlib's raw stream of `text`; flush_at: (position, Z_SYNC_FLUSH / Z_FULL_FLUSH) in mid-stream, ascending"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    raw, at = b"", 0
    for pos, mode in flush_at:
        raw += c.compress(text[at:pos]) + c.flush(mode)
        at = pos
    return raw + c.compress(text[at:]) + c.flush()


def member(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_at=(), extra_before: bytes = b"") -> bytes:
    return wrap(deflate(text, level, strategy, flush_at), zlib.crc32(text), len(text), extra_before)


def member_fits(text: bytes, level: int, strategy: int) -> bool:
    return 18 + len(deflate(text, level, strategy)) + 8 <= 65536


def bgzf(text: bytes, cut: int = BGZIP_CUT, level: int = 6, eof: bool = True) -> bytes:
    """a file as bgzip writes it: members of `cut` bytes of text, then the end-of-file marker"""
    out = b"".join(member(text[i:i + cut], level) for i in range(0, len(text), cut))
    return out + (EOF_MARKER if eof else b"")


def member_offsets(data: bytes):
    """the offsets of the members of a sound file, by BSIZE (BC first among the subfields), and the end"""
    off, at = [], 0
    while at < len(data):
        off.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    assert at == len(data)
    return off + [at]


# ---- texts ----
def fastq(n_records: int, seed: int = 5, read_len: int = 100) -> bytes:
    rnd = random.Random(seed)
    out = []
    for i in range(n_records):
        n = read_len if read_len > 0 else rnd.randrange(30, 151)
        out.append(b"@read%d/1\n%s\n+\n%s\n" % (i, bytes(rnd.choice(b"ACGT") for _ in range(n)), bytes(rnd.randrange(35, 74) for _ in range(n))))
    return b"".join(out)


def texts():
    """(name, text): the texts of the issue's list"""
    rnd = random.Random(11)
    fq = fastq(400)
    far = bytes(rnd.randrange(256) for _ in range(100))
    middle = bytes(rnd.choice(b"ACGTN") for _ in range(65536 - 200))
    return [("empty", b""), ("one_byte", b"A"), ("few_records", fastq(5, seed=3)), ("fastq_65280", fq[:65280]), ("fastq_65536", fq[:65536]),
            ("random_65280", bytes(rnd.randrange(256) for _ in range(65280))), ("i_run", b"I" * 65280), ("acgt", b"ACGT" * 4000),
            ("far_match", far + middle + far)]


# ---- members written bit by bit ----
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, n: int):      # n bits, least significant first (header fields, extra bits)
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int):      # a Huffman code, most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951's assignment"""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
# the code-length code of dynamic_header: 13 symbols of four bits, 6 of five (complete), no repeats needed
CL_LENGTHS = [4] * 13 + [5] * 6
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def block_header(b: Bits, btype: int, final: bool = True):
    b.put(1 if final else 0, 1)
    b.put(btype, 2)


def dynamic_header(b: Bits, lit_lengths, dist_lengths, final: bool = True, cl_lengths=None, symbols=None):
    """a dynamic block's header: every length as a plain symbol, or `symbols` = [(code-length symbol, extra value, extra bits)]"""
    cl_lengths = CL_LENGTHS if cl_lengths is None else cl_lengths
    block_header(b, 2, final)
    b.put(len(lit_lengths) - 257, 5)
    b.put(len(dist_lengths) - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(cl_lengths[s], 3)
    cl = canonical(cl_lengths)
    if symbols is None:
        symbols = [(ln, 0, 0) for ln in list(lit_lengths) + list(dist_lengths)]
    for s, extra, n_extra in symbols:
        b.code(*cl[s])
        b.put(extra, n_extra)


def hand_member(payload: bytes, text: bytes, isize=None, crc=None) -> bytes:
    return wrap(payload, zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


def fixed_literals(text: bytes) -> bytes:
    b = Bits()
    block_header(b, 1)
    for c in text:
        b.code(*FIXED_LIT[c])
    b.code(*FIXED_LIT[256])
    return b.bytes()


def dynamic_literals(text: bytes) -> bytes:
    """a dynamic block by this file's own encoder: the bytes of `text` and the end-of-block code in a complete code of nine bits or fewer"""
    used = sorted(set(text) | {256})
    if len(used) == 1:
        used = [0, 256]   # (a code of one symbol is not complete)
    k = len(used).bit_length() - 1
    n_long = 2 * (len(used) - (1 << k))   # complete: n_long symbols of k + 1 bits behind the others of k bits
    lit = [0] * 257
    for i, s in enumerate(used):
        lit[s] = k + 1 if i >= len(used) - n_long else k
    codes = canonical(lit)
    b = Bits()
    dynamic_header(b, lit, [0])
    for c in text:
        b.code(*codes[c])
    b.code(*codes[256])
    return b.bytes()


def stream_clause_members():
    """{clause name: a member that is refused by it}: one per stream clause, none of them what a compressor writes"""
    out = {}
    out["btype3"] = hand_member(b"\x07", b"")
    out["stored_len"] = hand_member(b"\x01\x01\x00\x00\x00A", b"A")
    out["stored_past"] = hand_member(b"\x01\x05\x00\xfa\xffAB", b"ABCDE")
    b = Bits()
    block_header(b, 2)
    b.put(30, 5); b.put(0, 5); b.put(0, 4)   # HLIT = 287
    b.put(0, 12)
    out["too_many_codes"] = hand_member(b.bytes(), b"")
    b = Bits()
    dynamic_header(b, [0] * 257, [0], cl_lengths=[1] * 19, symbols=[])   # nineteen codes of one bit
    out["code_lengths"] = hand_member(b.bytes() + b"\0\0", b"")
    cl = [0] * 19
    cl[0], cl[16] = 1, 1
    b = Bits()
    dynamic_header(b, [0] * 257, [0], cl_lengths=cl, symbols=[(16, 0, 2)])   # "repeat the last length" first of all
    out["repeat"] = hand_member(b.bytes() + b"\0\0", b"")
    cl = [0] * 19
    cl[0], cl[18] = 1, 1
    b = Bits()
    dynamic_header(b, [0] * 257, [0], cl_lengths=cl, symbols=[(18, 127, 7), (18, 109, 7)])   # 138 + 120 zeros: 258 lengths, none for 256
    out["no_eob"] = hand_member(b.bytes() + b"\0\0", b"")
    lit = [0] * 258   # 'A' and end-of-block in two bits, the length symbol 257 in one; no distance code at all
    lit[65], lit[256], lit[257] = 2, 2, 1
    codes = canonical(lit)
    b = Bits()
    dynamic_header(b, lit, [0])
    b.code(*codes[65]); b.code(*codes[257]); b.put(0, 9)
    out["bad_code"] = hand_member(b.bytes() + b"\0", b"AAAA")
    b = Bits()
    block_header(b, 1)
    b.code(*FIXED_LIT[286])
    out["litlen_sym"] = hand_member(b.bytes() + b"\0", b"")
    b = Bits()
    block_header(b, 1)
    b.code(*FIXED_LIT[65]); b.code(*FIXED_LIT[257]); b.code(*FIXED_DIST[30])
    out["dist_sym"] = hand_member(b.bytes() + b"\0", b"AAAA")
    b = Bits()
    block_header(b, 1)
    b.code(*FIXED_LIT[65]); b.code(*FIXED_LIT[257]); b.code(*FIXED_DIST[1]); b.code(*FIXED_LIT[256])   # length 3 at distance 2 behind one byte
    out["dist_before"] = hand_member(b.bytes(), b"AAAA")
    text = fastq(3, seed=9)
    raw = deflate(text)
    out["out_beyond"] = wrap(raw, zlib.crc32(text), len(text) - 10)
    out["end"] = wrap(raw + b"\0", zlib.crc32(text), len(text))
    out["length"] = wrap(raw, zlib.crc32(text), len(text) + 1)
    out["crc"] = wrap(raw, zlib.crc32(text) ^ 0x100, len(text))
    assert sorted(out) == sorted(STREAM_CLAUSES)
    return out


def container_clause_members():
    """{clause name: (bytes, n)}: headers that are refused; n = the bytes up to the end of the file"""
    good = member(b"ACGT")
    short = bytearray(member(b""))
    struct.pack_into("<H", short, 16, 20)    # BSIZE + 1 = 21 < 18 + 8
    big = bytearray(good)
    struct.pack_into("<I", big, len(big) - 4, 65537)
    plain_gzip = b"\x1f\x8b\x08\x00\0\0\0\0\0\xff" + deflate(b"ACGT") + struct.pack("<II", zlib.crc32(b"ACGT"), 4)
    no_bc = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0XY\x02\0\x00\x00" + deflate(b"ACGT") + struct.pack("<II", zlib.crc32(b"ACGT"), 4)
    return {"magic": (b"@r\nA\n+\nI\n", 9), "not_blocked": (no_bc, len(no_bc)), "method": (good[:2] + b"\x07" + good[3:], len(good)),
            "flags": (plain_gzip, len(plain_gzip)), "flags_name": (good[:3] + b"\x0c" + good[4:], len(good)), "short": (bytes(short), len(short)),
            "past_end": (good, len(good) - 1), "isize": (bytes(big), len(big))}
