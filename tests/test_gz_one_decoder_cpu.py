"""One deflate decoder (csrc/pf_inflate_core.hpp: inflate_codes, inflate_block) behind two drivers -- K-INFLATE's inflate_stream over a
BGZF member and K-GUNZIP's decode_piece over the pieces of a plain gzip stream -- without a GPU: both drivers give the same text and
refuse a broken stream by the same clause, and what the rule-level calls answer on sound, cut and bit-flipped streams is what they
answered before the two decoders became one."""
import hashlib
import os
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT

import gz_cases as gz
import gz_one_cases as one
import gzp_cases as gp

from ploidyfrost_amd import hostapi

# SHA-256 of what tests/cpp/gz_decode_dump.cpp printed for gz_one_cases.dump_records(False) at budget 3000 when it was compiled against the
# headers of the commit in front of the merge (two decoders: pf_inflate::inflate_codes / inflate_stream and pf_gunzip::piece_codes /
# decode_piece), 2052 inputs.  Recorded from that commit, not from the code under test.
DUMP_BUDGET = 3000
DUMP_INPUTS = 2052
DUMP_SHA256_BEFORE_THE_MERGE = "d076cb46596691825bd0d1a3e5f43ee0403ef8375826658503656079d25c2cb4"


def test_one_decoder_two_drivers_same_text():
    assert len(one.members()) >= 50
    for name, payload, text in one.members():
        clause, made, blocks = hostapi.inflate_member(payload, len(text))
        assert clause == 0 and made == text, name
        for piece in (64, 1 << 30):
            out, r, st, _ = hostapi.gunzip_call(payload, 0, b"", piece)
            assert r["clause"] == 0 and r["final"] == 1 and out == text, (name, piece)
            assert [st["blocks_stored"], st["blocks_fixed"], st["blocks_dynamic"]] == blocks, (name, piece)


def test_one_decoder_two_drivers_same_clause():
    """every refused stream of gzp_cases: the same clause number from both drivers.  (The clauses one driver alone has -- out_beyond and
    length for a member, piece_limit for a piece -- are not among these streams' clauses.)"""
    members = gz.stream_clause_members()
    refusals = gp.stream_refusals()
    assert len(refusals) == 10
    for name, bad in refusals.items():
        assert name not in ("out_beyond", "length", "piece_limit")
        isize = struct.unpack("<I", members[name][-4:])[0]
        clause, _, _ = hostapi.inflate_member(bad, isize)
        assert clause == gz.CLAUSE[name], name
        for piece in (64, 1 << 30):
            out, r, _, _ = hostapi.gunzip_call(bad, 0, b"", piece)
            assert r["clause"] == clause and out == b"", (name, piece)


def test_rule_level_answers_are_those_of_the_two_decoders(tmp_path):
    """tests/cpp/gz_decode_dump.cpp under the sanitizers (host code only, a program of its own) over the reduced corpus: every line it
    prints -- clause, bytes produced, end bit, block counters, hash of the text, for every stream whole, cut and with a bit flipped --
    hashes to what the two separate decoders printed."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "gz_decode_dump")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "gz_decode_dump.cpp"), "-o", exe], check=True)
    path = tmp_path / "records.bin"
    path.write_bytes(one.dump_records(False))
    r = subprocess.run([exe, str(path), str(DUMP_BUDGET)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    assert r.stdout.splitlines()[-1] == b"inputs %d" % DUMP_INPUTS
    assert hashlib.sha256(r.stdout).hexdigest() == DUMP_SHA256_BEFORE_THE_MERGE
