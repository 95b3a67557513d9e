"""K-INFLATE on the device (pf_inflate_bgzf through hipapi.Device.inflate_bgzf; csrc/pf_inflate.hip) against the host rule
(hostapi.inflate_bgzf, which tests/test_inflate_rule_cpu.py pins against zlib).  Bytes only: the texts, the statistics, the member
and the clause of every refusal.  The corrupt members are the ones the CPU tests and the sanitizer program have already passed through
the shared decoder (csrc/pf_inflate_core.hpp); the kernel's contract is to refuse them by name."""
import zlib

import numpy as np
import pytest
import torch

import gz_cases as gz

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def kinds():
    """one member of each kind of the CPU list: every text under the settings that give its stored, fixed and dynamic forms, a member of
    several blocks, one with a second subfield, the end-of-file marker: (members, texts)"""
    members, texts = [], []
    for name, text in gz.texts():
        for setting, level, strategy in (gz.SETTINGS[0], gz.SETTINGS[1], gz.SETTINGS[3]) if len(text) > 1000 else (gz.SETTINGS[3],):
            if gz.member_fits(text, level, strategy):
                members.append(gz.member(text, level, strategy))
                texts.append(text)
    fq = gz.fastq(200, seed=2)
    members.append(gz.member(fq, 6, flush_at=[(5000, zlib.Z_SYNC_FLUSH), (5000, zlib.Z_SYNC_FLUSH), (20000, zlib.Z_FULL_FLUSH)]))
    texts.append(fq)
    for setting, level, strategy in gz.SETTINGS[4:]:
        members.append(gz.member(fq, level, strategy))
        texts.append(fq)
    members.append(gz.member(b"@r\nACGT\n+\nIIII\n", extra_before=b"XY\x03\x00abc"))
    texts.append(b"@r\nACGT\n+\nIIII\n")
    members.append(gz.EOF_MARKER)
    texts.append(b"")
    return members, texts


def offsets(members):
    return np.cumsum([0] + [len(m) for m in members]).astype(np.uint64)


def host_stats(members):
    blocks = np.sum([hostapi.inflate_bgzf_member(m)[2] for m in members], axis=0) if members else [0, 0, 0]
    return [int(b) for b in blocks]


def test_one_member_of_each_kind(dev, kinds):
    members, texts = kinds
    assert 18 <= len(members) <= 30
    data = b"".join(members)
    want = hostapi.inflate_bgzf(data)
    assert want == b"".join(texts)
    out, stats = dev.inflate_bgzf(data, offsets(members))
    assert bytes(out) == want
    s, f, d = host_stats(members)
    assert stats == dict(members=len(members), bytes_in=len(data), bytes_out=len(want), blocks_stored=s, blocks_fixed=f, blocks_dynamic=d)
    assert s and f and d
    # the same on device pointers, the members at an odd address and the text to an odd address
    comp = torch.zeros(len(data) + 3, dtype=torch.uint8, device="cuda")
    comp[3:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    off = torch.from_numpy(offsets(members).astype(np.int64) + 3).cuda()
    buf = torch.full((len(want) + 9,), 0xA5, dtype=torch.uint8, device="cuda")
    dev.enable_timing(True)
    try:
        got, stats2 = dev.inflate_bgzf(comp, off, out=buf[1:], out_cap=len(want))
        ms, launches = dev.kernel_time(hipapi.K_INFLATE)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_INFLATE) == len(want)
    finally:
        dev.enable_timing(False)
    host = buf.cpu().numpy()
    assert bytes(host[1: 1 + len(want)]) == want and host[0] == 0xA5 and (host[1 + len(want):] == 0xA5).all()
    assert stats2 == dict(stats, bytes_in=len(data))


def test_300_small_members_with_empty_ones_between(dev):
    fq = gz.fastq(700, seed=13, read_len=0).split(b"\n@read")
    records = [fq[0] + b"\n"] + [b"@read" + r + b"\n" for r in fq[1:-1]] + [b"@read" + fq[-1]]
    members, at = [gz.EOF_MARKER], 0
    for i in range(300):
        n = 1 + i % 3
        members.append(gz.member(b"".join(records[at: at + n]), (1, 6, 9)[i % 3]))
        at += n
        if i % 7 == 0:
            members.append(gz.EOF_MARKER)
    members.append(gz.EOF_MARKER)
    data = b"".join(members)
    want = b"".join(records[:at])
    assert hostapi.inflate_bgzf(data) == want
    out, stats = dev.inflate_bgzf(data, offsets(members))
    assert bytes(out) == want and stats["members"] == len(members) and stats["bytes_out"] == len(want)
    s, f, d = host_stats(members)
    assert (stats["blocks_stored"], stats["blocks_fixed"], stats["blocks_dynamic"]) == (s, f, d)


def test_single_member_none_and_only_empty_ones(dev):
    text = gz.fastq(30, seed=1)
    m = gz.member(text)
    out, stats = dev.inflate_bgzf(m, [0, len(m)])
    assert bytes(out) == text and stats["members"] == 1 and stats["bytes_in"] == len(m)
    out, stats = dev.inflate_bgzf(b"", [0])
    assert len(out) == 0 and stats == dict.fromkeys(hipapi.INFLATE_STATS.names, 0)
    out, stats = dev.inflate_bgzf(gz.EOF_MARKER * 3, [0, 28, 56, 84])
    assert len(out) == 0 and stats["members"] == 3 and stats["blocks_fixed"] == 3


def test_out_cap_one_byte_short(dev):
    text = gz.fastq(900, seed=3)
    data = gz.bgzf(text)
    off = gz.member_offsets(data)
    buf = np.full(len(text) + 8, 0xA5, dtype=np.uint8)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(data, off, out=buf, out_cap=len(text) - 1)
    assert e.value.status == hipapi.PF_ERR_OVERFLOW and e.value.needed == len(text)
    assert (buf == 0xA5).all()
    out, _ = dev.inflate_bgzf(data, off, out=buf, out_cap=len(text))
    assert bytes(out) == text and (buf[len(text):] == 0xA5).all()


@pytest.mark.parametrize("name", gz.STREAM_CLAUSES)
def test_stream_clause_in_the_middle_of_ten_members(dev, name):
    good = [gz.member(gz.fastq(20 + i, seed=i)) for i in range(10)]
    bad = gz.stream_clause_members()[name]
    assert hostapi.inflate_bgzf_member(bad)[0] == gz.CLAUSE[name]
    members = good[:5] + [bad] + good[5:]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(b"".join(members), offsets(members))
    assert e.value.status == hipapi.PF_ERR_ARG and e.value.bad_member == 5
    assert str(e.value).endswith("pf_inflate_bgzf: member 5 of the call: " + hostapi.inflate_clause_text(gz.CLAUSE[name]))


def test_container_clauses_and_the_smallest_offender(dev):
    good = [gz.member(gz.fastq(20 + i, seed=i)) for i in range(6)]
    c = gz.container_clause_members()
    for name in ("method", "flags", "not_blocked", "short", "isize"):
        members = good[:3] + [c[name][0]] + good[3:]
        with pytest.raises(hipapi.DeviceError) as e:
            dev.inflate_bgzf(b"".join(members), offsets(members))
        assert e.value.bad_member == 3 and gz.CLAUSE_WORDS[name] in str(e.value), name
    s = gz.stream_clause_members()
    members = good[:2] + [s["crc"]] + good[2:4] + [s["btype3"], c["method"][0]] + good[4:]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(b"".join(members), offsets(members))
    assert e.value.bad_member == 2 and "CRC-32 mismatch" in str(e.value)      # the smallest, whichever stage refuses it
    members = good[:2] + [c["method"][0]] + good[2:4] + [s["btype3"]] + good[4:]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(b"".join(members), offsets(members))
    assert e.value.bad_member == 2 and "method is not 8" in str(e.value)
    members = good[:2] + [s["crc"]] + good[2:4] + [s["btype3"]] + good[4:]
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(b"".join(members), offsets(members))
    assert e.value.bad_member == 2 and "CRC-32 mismatch" in str(e.value)
    # a table that does not follow the members
    data = b"".join(good)
    off = offsets(good)
    off[3] += 1
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(data, off)
    assert e.value.bad_member == 2 and "member_off" in str(e.value)
    off = offsets(good)
    off[-1] += 5
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_bgzf(data, off)
    assert e.value.bad_member == 5 and "member_off" in str(e.value)
