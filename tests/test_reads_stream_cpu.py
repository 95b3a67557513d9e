"""The reads stream without a device (tests/cpp/test_reads_stream.cpp): host/pf_reads_stream.cpp and host/pf_gz_host.cpp linked against
stubs of the few pf_* calls they make, the step being the rule headers' host code.  Chunk edges, the long carry, the numbering per input,
the pair lock-step and the wind-down of the threads on an error, under the sanitizers (host code only: nothing of it is loaded into
Python or run on a GPU)."""
import os
import shutil
import subprocess

import pytest

import gz_cases as gz
import gzp_cases as gzp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ploidyfrost_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "test_reads_stream.cpp"), os.path.join(CSRC, "host", "pf_reads_stream.cpp"),
           os.path.join(CSRC, "host", "pf_gz_host.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(CSRC, "host"), "-I", os.path.join(ROOT, "include")]


def fixtures(d):
    """what the program reads: a text, the same as blocked gzip (members of 1 000 bytes of text) and as plain gzip, and a mate with as
    many records of other lengths"""
    text = gz.fastq(120, seed=31, read_len=0)
    for name, data in (("gz_text.fq", text), ("gz_text.fq.bgz", gz.bgzf(text, cut=1000)), ("gz_text.fq.gz", gzp.member(text)),
                       ("mate.fq", gz.fastq(120, seed=32, read_len=0))):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)


def build_and_run(tmp_path, name, sanitize):
    exe = str(tmp_path / name)
    subprocess.run(["g++"] + FLAGS + sanitize + SOURCES + ["-o", exe], check=True)
    work = tmp_path / (name + "_files")
    work.mkdir()
    fixtures(str(work))
    r = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", r.stdout + r.stderr


def test_reads_stream_program_under_address_and_undefined_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    build_and_run(tmp_path, "test_reads_stream", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_reads_stream_program_under_thread_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=thread", str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("g++ -fsanitize=thread does not link here")
    build_and_run(tmp_path, "test_reads_stream_tsan", ["-fsanitize=thread"])
