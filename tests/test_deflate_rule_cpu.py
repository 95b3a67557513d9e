"""The rule of K-DEFLATE (blocked-gzip output; csrc/pf_deflate_rule.hpp over csrc/pf_deflate_core.hpp, the encoder the kernel's threads run)
without a GPU: every member against Python's zlib and gzip and against the rule of K-INFLATE, the container's fields, the bound, the
block kinds, the sizes that show the match search at work (each taken from zlib's own output for that text), the cut into members, the
stand-alone program tests/cpp/test_deflate_rule.cpp under the sanitizers, and the declarations."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT

import gz_cases as gz
import gzo_cases as gzo

from ploidyfrost_amd import build, hipapi, hostapi


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_device()


TEXTS = gzo.member_texts()
MEMBERS = {}


def member_of(name):
    """the host rule's member of a text, made once"""
    if name not in MEMBERS:
        MEMBERS[name] = hostapi.deflate_member(dict(TEXTS)[name])
    return MEMBERS[name]


def zlib_size(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return len(gz.deflate(text, level, strategy))


@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_every_member_is_read_by_zlib_gzip_and_the_inflate_rule(name, text):
    member, kinds, literals, matches = member_of(name)
    assert zlib.decompress(member[18:-8], -15) == text
    assert gzip.decompress(member) == text
    clause, back, blocks = hostapi.inflate_bgzf_member(member)
    assert (clause, back) == (0, text)
    assert tuple(blocks) == kinds and sum(kinds) == 1   # one block a member, of the kind the rule says
    # the container, field by field
    assert member[:16] == bytes.fromhex("1f8b08040000000000ff060042430200")
    assert struct.unpack_from("<H", member, 16)[0] == len(member) - 1                                  # BSIZE
    assert struct.unpack_from("<II", member, len(member) - 8) == (zlib.crc32(text), len(text))         # CRC-32, ISIZE
    assert len(member) <= len(text) + 31
    assert literals + matches <= max(len(text), 0) and (matches == 0 or len(text) > 4)


def test_the_empty_text_is_the_end_of_file_marker():
    assert member_of("empty")[0] == gz.EOF_MARKER == hostapi.DEFLATE_EOF_MARKER


def test_block_kinds():
    assert member_of("random_65280")[1] == (1, 0, 0)                       # random bytes: one stored block, the bound met exactly
    assert len(member_of("random_65280")[0]) == 65280 + 31
    assert member_of("fibonacci")[1] == (0, 0, 1)
    freqs = [dict(TEXTS)["fibonacci"].count(bytes([c])) for c in range(256)]
    assert gzo.huffman_depth(freqs) > 15                                   # (the text's own code would not fit 15 bits)
    assert member_of("one_byte")[1] == (0, 1, 0)
    assert member_of("fastq_65280")[1] == (0, 0, 1)


def test_match_lengths_about_258():
    """a run of n bytes is one literal and matches of distance 1: 258 at most, the rest of at least four bytes or literals"""
    for n, (lit, mat) in {4: (4, 0), 257: (1, 1), 258: (1, 1), 259: (1, 1), 260: (2, 1), 261: (3, 1), 262: (4, 1), 65280: (1, 254)}.items():
        assert member_of("i_%d" % n)[2:] == (lit, mat), n
    assert member_of("literal_and_match")[2:] == (6, 1)
    assert member_of("acgt")[2:] == (4, 62)                                # 15 996 bytes at distance 4: 62 matches of 258


def test_distance_32768_is_taken_and_32769_is_not():
    near, far = member_of("far_32768"), member_of("far_32769")
    assert len(far[0]) - len(near[0]) > 50
    assert far[2] - near[2] > 90                                           # the copy's hundred bytes are literals in the one ...
    assert near[3] - far[3] in (1, 2)                                      # ... and a match (two, if a hash meets the filler) in the other


def test_sizes_that_a_broken_match_search_cannot_reach():
    texts = dict(TEXTS)
    for name in ("i_65280", "acgt"):   # zlib level 1: 0.46 % and 0.64 %; Z_HUFFMAN_ONLY: 12.5 % and 28 %
        assert len(member_of(name)[0]) < 0.02 * len(texts[name]), name
    binned = texts["binned_fastq"]
    assert len(member_of("binned_fastq")[0]) - 26 < zlib_size(binned, 6, zlib.Z_HUFFMAN_ONLY)


def test_a_text_of_three_members():
    text = gz.fastq(900, seed=12)[:2 * 65280 + 4321]
    data = hostapi.deflate_bgzf(text)
    assert gzip.decompress(data) == text
    assert data.endswith(gz.EOF_MARKER)
    off = gz.member_offsets(data)
    assert len(off) - 1 == 4
    cuts = [hostapi.inflate_parse_member(data[off[m]:])[1]["isize"] for m in range(4)]
    assert cuts == [65280, 65280, 4321, 0]
    assert hostapi.inflate_bgzf(data) == text
    assert hostapi.deflate_bgzf(text, eof=False) == data[:-28]
    assert hostapi.deflate_bgzf(b"") == gz.EOF_MARKER
    for name, long_text in gzo.texts():
        if len(long_text) > 65280:   # 65 281 bytes: a member of one byte behind the whole one
            d = hostapi.deflate_bgzf(long_text)
            assert gzip.decompress(d) == long_text and len(gz.member_offsets(d)) - 1 == 3, name
    with pytest.raises(ValueError):
        hostapi.deflate_member(b"A" * 65281)
    with pytest.raises(ValueError):
        hostapi.deflate_bgzf(b"A", member_text=0)


def test_members_of_other_cuts():
    text = gz.fastq(30, seed=13)
    for cut in (1, 7, 1000):
        data = hostapi.deflate_bgzf(text, member_text=cut)
        assert gzip.decompress(data) == text and len(gz.member_offsets(data)) - 2 == (len(text) + cut - 1) // cut


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_deflate_rule.cpp: the two headers and pf_inflate_rule.hpp alone, plain g++ with -fsanitize=address,undefined, over
    exact-size heap buffers: every text of gzo_cases (handed to it in a file) and every text cut at every length up to 600, deflated,
    inflated by the host rule and compared; and the code-length limit on frequencies that Huffman's construction takes past it (host
    code only: nothing of it is loaded into Python or run on a GPU)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "test_deflate_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_deflate_rule.cpp"), "-o", exe], check=True)
    path = tmp_path / "texts.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(t)) + t for _, t in gzo.texts()))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_entry_points_are_declared():
    L = hostapi.load_library()
    for s in ("pfh_deflate_member", "pfh_deflate_bound"):
        assert s in hostapi.DECLARED_SYMBOLS and hasattr(L, s)
    assert L.pfh_deflate_bound(65281, 65280) == 65281 + 62 and L.pfh_deflate_bound(0, 65280) == 0
    assert "pf_deflate_bgzf" in hipapi.DECLARED_SYMBOLS
    D = hipapi.load_library()
    assert hasattr(D, "pf_deflate_bgzf")
    assert hipapi.K_DEFLATE == hipapi.K_FASTA + 1 and D.pf_kernel_name(hipapi.K_DEFLATE) == b"k_deflate"
    with open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")) as f:
        text = f.read()
    assert "PF_K_DEFLATE" in text.split("PF_K_FASTA,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    at = text.index("int pf_deflate_bgzf(")
    decl = " ".join(text[at: text.index(";", at)].split())
    assert decl == ("int pf_deflate_bgzf(pf_ctx *, const char *text, uint64_t n_bytes, uint32_t member_text, uint8_t *out, uint64_t out_cap, "
                    "uint64_t *out_bytes, uint64_t *member_off, pf_deflate_stats *stats)")
    assert hipapi.DEFLATE_STATS.itemsize == 64
    assert hipapi.DEFLATE_STATS.names == ("members", "bytes_in", "bytes_out", "blocks_stored", "blocks_fixed", "blocks_dynamic", "literals", "matches")
    with open(os.path.join(ROOT, "ploidyfrost_amd", "csrc", "Makefile")) as f:
        assert "pf_deflate.hip" in f.read().split("DEV_SRC")[1].split("\n")[0]
