"""The rule of K-INFLATE (blocked gzip; csrc/pf_inflate_rule.hpp over csrc/pf_inflate_core.hpp, the decoder the kernel's lanes run)
without a GPU: inflate_member and crc32 against Python's zlib over every kind of block the compressor writes and the edge texts, the
member header, every refusal provoked by a hand-made member and named, single-bit corruption of a dynamic member, the stand-alone
program tests/cpp/test_inflate_rule.cpp under the sanitizers, and the declarations."""
import gzip
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT

import gz_cases as gz

from ploidyfrost_amd import build, hipapi, hostapi


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


TEXTS = gz.texts()


def payload_of(member):
    clause, h = hostapi.inflate_parse_member(member)
    assert clause == 0
    return member[h["payload_off"]: h["member_len"] - 8], h


# ---- against zlib ----

@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_members_of_every_setting_against_zlib(name, text):
    kinds = set()
    for setting, level, strategy in gz.SETTINGS:
        if not gz.member_fits(text, level, strategy):   # (65 536 stored bytes and their headers are more than a member holds)
            assert level == 0 or name.startswith("random"), (name, setting)
            continue
        m = gz.member(text, level, strategy)
        assert gzip.decompress(m) == text
        payload, h = payload_of(m)
        assert h["isize"] == len(text) and h["crc"] == zlib.crc32(text) and h["member_len"] == len(m)
        clause, out, blocks = hostapi.inflate_member(payload, len(text))
        assert clause == 0 and out == text, (name, setting, hostapi.inflate_clause_text(clause))
        assert hostapi.inflate_bgzf_member(m)[:2] == (0, text)
        kinds |= {k for k, n in zip(("stored", "fixed", "dynamic"), blocks) if n}
        if text and not name.startswith("random"):   # (random bytes are stored whatever the strategy)
            first = {"level0": "stored", "fixed": "fixed"}.get(setting)
            if first:
                assert blocks[("stored", "fixed").index(first)] >= 1 and blocks[2] == 0, (name, setting, blocks)
    if len(text) > 1000 and not name.startswith("random"):
        assert kinds >= {"fixed", "dynamic"} and ("stored" in kinds) == gz.member_fits(text, 0, zlib.Z_DEFAULT_STRATEGY), (name, kinds)
    assert hostapi.inflate_crc32(text) == zlib.crc32(text)
    for lanes in (1, 3, 64):
        assert hostapi.inflate_crc32(text, lanes) == zlib.crc32(text), lanes


def test_the_sizes_the_issue_states():
    texts = dict(TEXTS)
    stored = gz.member(texts["random_65280"], 0)   # (65 326 bytes with zlib's four stored blocks; other builds of it cut fewer)
    assert 65280 + 26 + 2 * 5 <= len(stored) <= 65326 and hostapi.inflate_bgzf_member(stored)[2][0] >= 2
    assert hostapi.inflate_bgzf_member(gz.member(texts["random_65280"], 6))[2][0] >= 1
    assert len(gz.member(texts["i_run"])) <= 106
    assert gz.member(b"") == gz.EOF_MARKER and len(gz.EOF_MARKER) == 28
    clause, h = hostapi.inflate_parse_member(gz.EOF_MARKER)
    assert clause == 0 and h == dict(payload_off=18, member_len=28, crc=0, isize=0)
    assert hostapi.inflate_bgzf_member(gz.EOF_MARKER) == (0, b"", [0, 1, 0])


def test_several_blocks_in_one_member():
    text = gz.fastq(200, seed=2)
    cuts = [(5000, zlib.Z_SYNC_FLUSH), (5000, zlib.Z_SYNC_FLUSH), (20000, zlib.Z_FULL_FLUSH), (30001, zlib.Z_SYNC_FLUSH)]
    m = gz.member(text, 6, flush_at=cuts)
    clause, out, blocks = hostapi.inflate_bgzf_member(m)
    assert clause == 0 and out == text
    assert blocks[0] >= 4 and blocks[1] + blocks[2] >= 4, blocks   # an empty stored block behind every flush, two of them at 5000


def test_concatenated_file_and_far_matches():
    text = gz.fastq(1500, seed=4, read_len=0)
    data = gz.bgzf(text)
    assert gzip.decompress(data) == text
    off = gz.member_offsets(data)
    assert len(off) - 1 == (len(text) + gz.BGZIP_CUT - 1) // gz.BGZIP_CUT + 1
    assert hostapi.inflate_bgzf(data) == text
    far = dict(TEXTS)["far_match"]
    assert len(far) == 65536 and far[:100] == far[-100:]
    assert hostapi.inflate_bgzf_member(gz.member(far, 9))[:2] == (0, far)


def test_own_encoders_are_sound():
    """the members written bit by bit in gz_cases are read by zlib as well: what the refusals below are built with"""
    for text in (b"", b"A", b"ACGTACGTNNNN\n", bytes(range(256))):
        for payload in (gz.fixed_literals(text), gz.dynamic_literals(text)):
            assert zlib.decompress(payload, -15) == text
            m = gz.hand_member(payload, text)
            assert hostapi.inflate_bgzf_member(m)[:2] == (0, text)


# ---- the member header ----

def test_parse_member_fields_and_subfields():
    text = b"@r\nACGT\n+\nIIII\n"
    m = gz.member(text, extra_before=b"XY\x03\x00abc")
    clause, h = hostapi.inflate_parse_member(m)
    assert clause == 0 and h == dict(payload_off=12 + 7 + 6, member_len=len(m), crc=zlib.crc32(text), isize=len(text))
    assert hostapi.inflate_bgzf_member(m)[:2] == (0, text)
    assert gzip.decompress(m) == text


def test_container_clauses_by_name():
    for name, (data, n) in gz.container_clause_members().items():
        want = name.split("_name")[0]
        clause, _ = hostapi.inflate_parse_member(data, n)
        assert clause == gz.CLAUSE[want], (name, gz.CLAUSES[clause])
        assert gz.CLAUSE_WORDS[want] in hostapi.inflate_clause_text(clause)
    text = hostapi.inflate_clause_text(gz.CLAUSE["not_blocked"])
    assert "bgzip" in text and "decompress" in text


def test_file_clause_for_the_preflight():
    c = gz.container_clause_members()
    good = gz.bgzf(gz.fastq(3))
    assert hostapi.inflate_file_clause(b"@r\nA\n+\nI\n") == (0, 0)
    assert hostapi.inflate_file_clause(b">r\nA\n") == (0, 0)          # (FASTA is the plain path's refusal)
    assert hostapi.inflate_file_clause(b"") == (0, 0)
    assert hostapi.inflate_file_clause(good) == (1, 0)
    assert hostapi.inflate_file_clause(good[:65536], 10 ** 9) == (1, 0)
    for name in ("not_blocked", "method", "flags", "short"):
        assert hostapi.inflate_file_clause(c[name][0]) == (2, gz.CLAUSE[name]), name
    assert hostapi.inflate_file_clause(good[:40]) == (2, gz.CLAUSE["past_end"])     # a first member that runs past the file's end
    assert hostapi.inflate_file_clause(good[:10]) == (2, gz.CLAUSE["past_end"])
    assert hostapi.inflate_file_clause(c["isize"][0]) == (1, 0)                     # a member clause: named with its number once the stream runs


# ---- the stream's refusals ----

def test_stream_clauses_by_name():
    for name, m in gz.stream_clause_members().items():
        clause, text, _ = hostapi.inflate_bgzf_member(m)
        assert clause == gz.CLAUSE[name] and text == b"", (name, gz.CLAUSES[clause])
        assert gz.CLAUSE_WORDS[name] in hostapi.inflate_clause_text(clause), name
        with pytest.raises((zlib.error, OSError, EOFError)):   # (Python's gzip refuses every one of them too)
            gzip.decompress(m)
    with pytest.raises(ValueError) as e:
        hostapi.inflate_bgzf(gz.member(b"ACGT") + gz.stream_clause_members()["btype3"])
    assert str(e.value) == "member 2, byte %d: a deflate block of type 3" % len(gz.member(b"ACGT"))


def corrupt_outcomes(member, text, flips):
    """every flip ends in a clause (CRC mismatch among them) or, where the bit does not matter, in the same bytes: never in other bytes
    with a matching CRC, never outside the buffers (hostapi.inflate_member checks its guard bytes)"""
    payload, h = payload_of(member)
    outcomes = {}
    for bits in flips:
        bad = bytearray(payload)
        for bit in bits:
            bad[bit // 8] ^= 1 << (bit % 8)
        clause, out, _ = hostapi.inflate_member(bytes(bad), h["isize"])
        assert len(out) <= h["isize"]
        whole = bytearray(member)
        whole[h["payload_off"]: h["member_len"] - 8] = bad
        c2, out2, _ = hostapi.inflate_bgzf_member(bytes(whole))
        assert (c2 == 0 and out2 == text) or (c2 != 0 and out2 == b""), (bits, gz.CLAUSES[c2])
        assert c2 == (clause or (0 if out == text else gz.CLAUSE["crc"])), (bits, clause, c2)
        outcomes[gz.CLAUSES[c2]] = outcomes.get(gz.CLAUSES[c2], 0) + 1
    return outcomes


def test_every_flip_of_the_first_200_bits_is_refused_or_harmless():
    text = gz.fastq(40, seed=6)
    m = gz.member(text, 6)
    assert hostapi.inflate_bgzf_member(m)[2] == [0, 0, 1]   # one dynamic block: the first 200 bits are its header and code lengths
    outcomes = corrupt_outcomes(m, text, [[b] for b in range(200)])
    assert outcomes.get("none", 0) <= 5 and len(outcomes) >= 5, outcomes
    rnd = random.Random(20)
    n_bits = 8 * (len(m) - 26)
    more = corrupt_outcomes(m, text, [rnd.sample(range(n_bits), rnd.randrange(1, 4)) for _ in range(300)])
    assert more.get("none", 0) == 0 or more["none"] < 30, more


def test_flips_of_stored_and_fixed_members():
    text = gz.fastq(10, seed=8)
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
        corrupt_outcomes(gz.member(text, level, strategy), text, [[b] for b in range(120)])


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_inflate_rule.cpp: the two headers alone, plain g++ with -fsanitize=address,undefined, over exact-size heap buffers:
    the hand-made members and the corrupt-member loop (host code only: nothing of it is loaded into Python or run on a GPU).  The
    dynamic member it corrupts as well is handed to it in a file."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "test_inflate_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_inflate_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
    text = gz.fastq(40, seed=6)
    members = [gz.member(text, 6), gz.member(text, 6, zlib.Z_FIXED), gz.member(text, 0), gz.member(dict(TEXTS)["far_match"], 9)]
    path = tmp_path / "members.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(m)) + m for m in members))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


# ---- names ----

def test_entry_points_are_declared():
    L = hostapi.load_library()
    for s in ("pfh_inflate_parse_member", "pfh_inflate_member", "pfh_inflate_bgzf_member", "pfh_inflate_crc32", "pfh_inflate_crc32_sliced",
              "pfh_inflate_file_clause", "pfh_inflate_clause_text"):
        assert s in hostapi.DECLARED_SYMBOLS and hasattr(L, s)
    assert "pf_inflate_bgzf" in hipapi.DECLARED_SYMBOLS
    D = hipapi.load_library()
    assert hipapi.K_INFLATE == hipapi.K_TRIMCOUNT + 1 and D.pf_kernel_name(hipapi.K_INFLATE) == b"k_inflate"
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_INFLATE" in text.split("PF_K_TRIMCOUNT,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    at = text.index("int pf_inflate_bgzf(")
    decl = " ".join(text[at: text.index(";", at)].split())
    assert decl == ("int pf_inflate_bgzf(pf_ctx *, const uint8_t *comp, uint64_t n_bytes, const uint64_t *member_off, uint64_t n_members, char *out, "
                    "uint64_t out_cap, uint64_t *out_bytes, pf_inflate_stats *stats, uint64_t *bad_member)")
    assert hipapi.INFLATE_STATS.itemsize == 48
    for i, name in enumerate(gz.CLAUSES[1:], 1):
        assert gz.CLAUSE_WORDS[name] in hostapi.inflate_clause_text(i), name
    with open(os.path.join(ROOT, "ploidyfrost_amd", "csrc", "Makefile")) as f:
        assert "pf_inflate.hip" in f.read().split("DEV_SRC")[1].split("\n")[0]
