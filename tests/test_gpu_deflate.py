"""K-DEFLATE on the device (pf_deflate_bgzf, Device.deflate_bgzf) against the host rule (hostapi.deflate_member, the same
pf_deflate_core.hpp run as lane 0 of 1): the bytes member for member over every text of gzo_cases, the way back through K-INFLATE, other
cuts, device pointers at odd alignments, the bound, the refusals and the counters."""
import gzip

import numpy as np
import pytest
import torch

import gz_cases as gz
import gzo_cases as gzo

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu

TEXTS = gzo.texts()
HOST = {}


def host_members(text, cut=65280):
    """the host rule's members of a text, made once: [(member, kinds, literals, matches)]"""
    key = (text, cut)
    if key not in HOST:
        HOST[key] = [hostapi.deflate_member(text[at:at + cut]) for at in range(0, len(text), cut)]
    return HOST[key]


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def check_against_host(data, off, stats, text, cut=65280):
    want = host_members(text, cut)
    off = [int(x) for x in off]
    assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(data)
    for m, (member, _, _, _) in enumerate(want):
        assert bytes(data[off[m]:off[m + 1]]) == member, "member %d" % m
    assert stats["members"] == len(want) and stats["bytes_in"] == len(text) and stats["bytes_out"] == len(data)
    assert (stats["blocks_stored"], stats["blocks_fixed"], stats["blocks_dynamic"]) == tuple(sum(w[1][k] for w in want) for k in range(3))
    assert stats["blocks_stored"] + stats["blocks_fixed"] + stats["blocks_dynamic"] == stats["members"]
    assert stats["literals"] == sum(w[2] for w in want) and stats["matches"] == sum(w[3] for w in want)


@pytest.mark.parametrize("name,text", TEXTS, ids=[t[0] for t in TEXTS])
def test_every_text_gives_the_bytes_of_the_host_rule_and_inflates_back(dev, name, text):
    data, off, stats = dev.deflate_bgzf(text)
    check_against_host(data, off, stats, text)
    if text:
        d_data = torch.from_numpy(np.array(data)).cuda()
        d_text = torch.zeros(len(text), dtype=torch.uint8, device="cuda")
        back, _ = dev.inflate_bgzf(d_data, off, out=d_text)
        assert bytes(back.cpu().numpy()) == text


def test_seventy_members_of_a_thousand_bytes(dev):
    text = gz.fastq(400, seed=21)[:70000]
    assert len(text) == 70000
    data, off, stats = dev.deflate_bgzf(text, member_text=1000)
    assert stats["members"] == 70
    check_against_host(data, off, stats, text, 1000)
    assert bytes(data) == hostapi.deflate_bgzf(text, member_text=1000, eof=False)
    assert gzip.decompress(bytes(data)) == text


def test_sixty_five_members_of_one_byte(dev):
    text = gz.fastq(1, seed=22)[:65]
    data, off, stats = dev.deflate_bgzf(text, member_text=1)
    assert stats["members"] == 65 and [int(x) for x in off] == [29 * m for m in range(66)]
    check_against_host(data, off, stats, text, 1)


@pytest.mark.parametrize("shift", [1, 3])
def test_device_pointers_at_odd_alignments(dev, shift):
    text = gzo.binned_fastq(65280 + 2000, seed=23)
    d_buf = torch.zeros(len(text) + 8, dtype=torch.uint8, device="cuda")
    d_buf[shift:shift + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((len(text) + 62 + 8 + shift,), 0xA5, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(3, dtype=torch.int64, device="cuda")
    data, off, stats = dev.deflate_bgzf(d_buf[shift:shift + len(text)], out=d_out[shift:shift + len(text) + 62], member_off=d_off)
    check_against_host(data.cpu().numpy(), d_off.cpu().numpy(), stats, text)
    whole = d_out.cpu().numpy()
    assert (whole[:shift] == 0xA5).all() and (whole[shift + len(data):] == 0xA5).all()   # nothing outside the members is written


def test_out_cap_below_the_bound_is_an_overflow_with_the_bound(dev):
    text = gz.fastq(700, seed=24)[:65281]
    bound = len(text) + 2 * 31
    with pytest.raises(hipapi.DeviceError) as e:
        dev.deflate_bgzf(text, out=np.zeros(bound - 1, dtype=np.uint8))
    assert e.value.status == hipapi.PF_ERR_OVERFLOW and str(bound) in str(e.value) and "pf_deflate_bgzf" in str(e.value)
    data, _, _ = dev.deflate_bgzf(text, out=np.zeros(bound, dtype=np.uint8))
    assert gzip.decompress(bytes(data)) == text


def test_no_text_gives_no_member(dev):
    data, off, stats = dev.deflate_bgzf(b"")
    assert len(data) == 0 and [int(x) for x in off] == [0] and stats["members"] == 0 and stats["bytes_out"] == 0


@pytest.mark.parametrize("member_text", [0, 65281])
def test_member_text_out_of_range_is_refused_by_name(dev, member_text):
    with pytest.raises(hipapi.DeviceError) as e:
        dev.deflate_bgzf(b"ACGT" * 10, member_text=member_text, out=np.zeros(4096, dtype=np.uint8))
    assert e.value.status == hipapi.PF_ERR_ARG and "member_text" in str(e.value) and str(member_text) in str(e.value)


def test_timed_as_one_launch_with_bytes_of_text_as_unit(dev):
    text = gz.fastq(100, seed=25)
    dev.reset_timing()
    dev.enable_timing(True)
    try:
        dev.deflate_bgzf(text)
        ms, launches = dev.kernel_time(hipapi.K_DEFLATE)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_DEFLATE) == len(text)
    finally:
        dev.enable_timing(False)
