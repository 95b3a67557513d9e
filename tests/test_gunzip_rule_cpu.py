"""The rule of K-GUNZIP (plain gzip; csrc/pf_gunzip_rule.hpp over csrc/pf_gunzip_core.hpp, the code the kernel's lanes run) without a
GPU: one call and whole files against Python's zlib on the streams A - G for every piece stride, the piece counts the issue states,
the search for block starts, the container and every clause by name, files fed block by block with the carry, the stand-alone program
tests/cpp/test_gunzip_rule.cpp under the sanitizers, and the declarations."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from conftest import ROOT

import gz_cases as gz
import gzp_cases as gp

from ploidyfrost_amd import hipapi, hostapi


def test_one_call_against_zlib_on_every_stream_and_stride():
    for name, (stream, text) in gp.streams().items():
        assert zlib.decompress(stream, -15) == text
        for piece in gp.PIECES:
            out, r, st, win = hostapi.gunzip_call(stream, 0, b"", piece)
            assert out == text and r["clause"] == 0 and r["final"] == 1 and r["out_bytes"] == len(text), (name, piece)
            assert (r["end_bit"] + 7) // 8 == len(stream) and win == text[-32768:], (name, piece)
            assert r["crc_raw"] ^ zlib.crc32(b"\0" * len(text)) == zlib.crc32(text), (name, piece)
            assert st["pieces_live"] + st["pieces_dead"] == st["pieces_found"] and st["bytes_out"] == len(text) and st["bytes_in"] == len(stream)


def test_the_streams_look_as_the_issue_says():
    s = gp.streams()
    call = lambda name, piece: hostapi.gunzip_call(s[name][0], 0, b"", piece)[2]   # noqa: E731
    assert len(s["A"][1]) == 430890 and len(s["A"][0]) == 227996 and len(s["B"][0]) == 280307
    a = call("A", 16384)
    assert (a["blocks_stored"], a["blocks_fixed"], a["blocks_dynamic"]) == (0, 0, 14) and a["pieces_live"] >= 8 and a["markers"] > 0
    b = call("B", 1024)
    assert (b["blocks_fixed"], b["blocks_dynamic"]) == (1, 1806) and b["pieces_live"] >= 200
    # every block start behind the first 64 bytes is found when every bit is searched, and nothing else: 13 non-final starts, all live
    every = call("A", 64)
    assert every["pieces_found"] == 13 and every["pieces_dead"] == 0
    assert call("C", 1024)["markers"] > 0 and call("C", 1024)["pieces_live"] >= 16
    assert call("D_flush", 1024)["blocks_stored"] >= 80 and call("D_block", 1024)["blocks_dynamic"] >= 80
    for name in ("E_stored", "E_fixed"):
        e = call(name, 64)
        assert e["pieces_found"] == 1 and e["pieces_live"] == 1 and e["markers"] == 0
    assert call("E_stored", 64)["blocks_stored"] >= 7 and call("E_fixed", 64)["blocks_fixed"] >= 2


def test_candidates_are_dynamic_block_headers():
    stream, _ = gp.streams()["A"]
    assert hostapi.gunzip_candidate(stream, 0)
    hits = [bit for bit in range(1, 4000) if hostapi.gunzip_candidate(stream, bit)]
    assert hits == []
    fixed, _ = gp.streams()["E_fixed"]
    assert not hostapi.gunzip_candidate(fixed, 0) and not hostapi.gunzip_candidate(gp.raw(b"ACGT" * 100), 0)   # fixed; final
    assert not hostapi.gunzip_candidate(stream[:40], 0) and not hostapi.gunzip_candidate(b"", 0) and not hostapi.gunzip_candidate(stream, 8 * len(stream) - 2)


def test_files_block_by_block():
    for name, (data, text) in gp.files().items():
        for piece, block in ((0, 0), (64, 4096), (1024, 1000)):
            st = {}
            assert hostapi.gunzip_member(data, piece, block, stats=st) == text, (name, piece, block)
            assert st["bytes_out"] == len(text)
    # every edge of a small file of three members, one of them empty, at blocks of a few bytes
    t1, t3 = gz.fastq(6, seed=1), gz.fastq(3, seed=2)
    small = gp.member(t1, head=gp.header(name=b"n", extra=b"AB\x01\x00z", comment=b"c", hcrc=True)) + gp.member(b"") + gp.member(t3, gp.raw(t3, 6, 8, zlib.Z_FIXED))
    for piece, block in ((64, 1), (64, 7), (1024, 100)):
        assert hostapi.gunzip_member(small, piece, block) == t1 + t3, (piece, block)
    stream, text = gp.streams()["B"]
    whole = gp.member(text, stream, gp.header(name=b"b.fq")) + gp.member(text[:5000])
    assert hostapi.gunzip_member(whole, 1024, 4096) == text + text[:5000]
    assert hostapi.gunzip_member(whole, 0, 70000) == text + text[:5000]


def refusal(data, **k):
    with pytest.raises(ValueError) as e:
        hostapi.gunzip_member(data, **k)
    return e.value.clause, e.value.member, e.value.byte


def test_every_clause_by_name():
    a = gz.fastq(300, seed=1)
    good = gp.member(a)
    two = good + gp.member(gz.fastq(20, seed=2))
    C = gp.CLAUSE
    assert refusal(b"\x1f\x8b\x07" + good[3:]) == (C["method"], 0, 0)
    assert refusal(b"\x1f\x8b\x08\x40" + good[4:]) == (C["reserved_flag"], 0, 0)
    assert refusal(gp.header(name=b"abcdef")[:14]) == (C["header_past"], 0, 0)
    assert refusal(good + gp.header(extra=b"12345")[:13]) == (C["header_past"], 1, len(good))
    assert refusal(good[:len(good) // 2]) [0] == C["cut_block"]
    assert refusal(good[:-3]) == (C["cut_trailer"], 0, len(good) - 8)
    assert refusal(good[:-8]) == (C["cut_trailer"], 0, len(good) - 8)
    assert refusal(two[:-4] + struct.pack("<I", 7)) == (C["length"], 1, len(two) - 4)
    assert refusal(two[:-8] + struct.pack("<I", 7) + two[-4:]) == (C["crc"], 1, len(two) - 8)
    assert refusal(good + b"@r1\n") == (C["trailing"], 1, len(good))
    assert refusal(good + b"\0" * 20) == (C["trailing"], 1, len(good))
    stream, text = gp.streams()["A"]
    assert refusal(gp.member(text, stream), piece_bytes=64, block_bytes=2000, carry_max=9000) == (C["block_too_large"], 0, 10)
    assert hostapi.gunzip_member(gp.member(text, stream), 64, 2000, 40000) == text
    prefix, ptext = gp.sound_prefix()
    for name, bad in gp.stream_refusals().items():
        assert refusal(gp.HEADER + bad) == (C[name], 0, 10), name
        if name != "dist_before":
            assert refusal(good + gp.HEADER + prefix + bad, block_bytes=3000) == (C[name], 1, len(good) + 10 + len(prefix)), name
        assert gp.CLAUSE[name] == gz.CLAUSE[name] and hostapi.gunzip_clause_text(C[name]) == hostapi.inflate_clause_text(C[name])
    for name in gp.CLAUSES:
        assert hostapi.gunzip_clause_text(C[name]) not in ("no refusal", ""), name
    assert "ISIZE mod 2^32" in hostapi.gunzip_clause_text(C["length"])
    # a window reaches 32 768 bytes back and no further: the distance of a second member does not reach into the first
    far = gp.stream_refusals()["dist_before"]
    assert refusal(good + gp.HEADER + far + gp.trailer(b"AAAA")) == (C["dist_before"], 1, len(good) + 10)


def test_the_first_bytes_of_a_file():
    text = gz.fastq(20, seed=5)
    kinds = {"text": 0, "bgzf": 1, "refused": 2, "gzip": 3}
    assert hostapi.gunzip_file_kind(text) == (kinds["text"], 0)
    assert hostapi.gunzip_file_kind(gz.bgzf(text)) == (kinds["bgzf"], 0)
    assert hostapi.gunzip_file_kind(gp.member(text)) == (kinds["gzip"], 0)
    assert hostapi.gunzip_file_kind(gp.member(text, head=gp.header(name=b"x", extra=b"AB\x01\x00z"))) == (kinds["gzip"], 0)
    nobc = gz.container_clause_members()["not_blocked"][0]
    assert hostapi.gunzip_file_kind(nobc) == (kinds["gzip"], 0) and hostapi.inflate_file_clause(nobc) == (2, gz.CLAUSE["not_blocked"])
    assert hostapi.gunzip_file_kind(b"\x1f\x8b\x09\x00" + b"\0" * 20) == (kinds["refused"], gp.CLAUSE["method"])
    assert hostapi.gunzip_file_kind(b"\x1f\x8b\x08\x80" + b"\0" * 20) == (kinds["refused"], gp.CLAUSE["reserved_flag"])
    assert hostapi.gunzip_file_kind(b"\x1f\x8b\x08\x08\0\0\0\0\0\3abc") == (kinds["refused"], gp.CLAUSE["header_past"])
    assert hostapi.gunzip_file_kind(b"\x1f\x8b\x08\x08\0\0\0\0\0\3abc", file_size=100) == (kinds["gzip"], 0)
    cut = gz.bgzf(text)[:40]
    assert hostapi.gunzip_file_kind(cut) == hostapi.inflate_file_clause(cut) == (kinds["refused"], gz.CLAUSE["past_end"])   # blocked gzip keeps its own refusals


def test_standalone_rule_program_under_the_sanitizers(tmp_path):
    """tests/cpp/test_gunzip_rule.cpp: the headers alone, plain g++ with -fsanitize=address,undefined, over exact-size heap buffers (host
    code only: nothing of it is loaded into Python or run on a GPU).  The streams it needs from zlib are handed to it in a file."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "test_gunzip_rule")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ploidyfrost_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_gunzip_rule.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr
    small = gz.fastq(6, seed=6)
    tiny = gz.fastq(3, seed=8, read_len=60)
    flip = gp.member(tiny, head=gp.header(name=b"t.fq"))
    assert 250 <= len(flip) <= 350
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    blocks = c.compress(small[:700]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(small[700:]) + c.flush()
    records = [(1, gp.member(small, blocks, gp.header(name=b"s.fq", comment=b"c"))), (2, small), (3, flip), (2, tiny)]
    records += [(4, bytes([gp.CLAUSE[name]]) + bad) for name, bad in gp.stream_refusals().items()]
    records.append((5, gp.sound_prefix()[0]))
    path = tmp_path / "records.bin"
    path.write_bytes(b"".join(struct.pack("<II", tag, len(b)) + b for tag, b in records))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_names():
    D = hipapi.load_library()
    assert hipapi.K_GUNZIP == hipapi.K_INFLATE + 1 and D.pf_kernel_name(hipapi.K_GUNZIP) == b"k_gunzip"
    text = open(os.path.join(ROOT, "include", "ploidyfrost_hip.h")).read()
    assert "PF_K_GUNZIP" in text.split("PF_K_INFLATE,")[1].split("PF_K_COUNT_")[0]   # appended: the values of old stay
    assert "pf_inflate_gzip" in hipapi.DECLARED_SYMBOLS and {"pfh_gunzip_call", "pfh_gunzip_file"} <= set(hostapi.DECLARED_SYMBOLS)
    core = open(os.path.join(ROOT, "ploidyfrost_amd", "csrc", "pf_gunzip_core.hpp")).read()
    assert '#include "pf_inflate_core.hpp"' in core and "CLAUSE_RESERVED_FLAG = pf_inflate::CLAUSE_COUNT_" in core
    assert hipapi.GUNZIP_RESULT.itemsize == 40 and hipapi.GUNZIP_STATS.itemsize == 9 * 8 + 5 * 8
    assert hostapi._gz_mode(False) == 0 and hostapi._gz_mode(True) == 1 and hostapi._gz_mode("plain") == 2
    with pytest.raises(ValueError):
        hostapi._gz_mode("bgzf")
