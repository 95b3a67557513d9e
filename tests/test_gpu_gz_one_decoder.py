"""The one deflate decoder (csrc/pf_inflate_core.hpp) and the one window in LDS (csrc/pf_gz_dev.hpp: GzIn) behind K-INFLATE and K-GUNZIP
on the device: the window at its first two refill points for every alignment of the compressed bytes, with guard bytes around them,
and both kernels on the same members against the host rule.  The cases are gz_one_cases'."""
import zlib

import pytest
import torch

import gz_cases as gz
import gz_one_cases as one

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def _painted(data: bytes, first_at: int, shift: int):
    """a device buffer of 0xA5 with `data` in it so that its byte `first_at` lies `shift` bytes past a dword boundary -> (buffer, offset)"""
    off = GUARD + (shift - first_at - GUARD) % 4
    buf = torch.full((off + len(data) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0 and (buf.data_ptr() + off + first_at) % 4 == shift
    buf[off: off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf, off


def _untouched(buf, off: int, data: bytes):
    host = buf.cpu().numpy()
    return (host[:off] == 0xA5).all() and (host[off + len(data):] == 0xA5).all() and host[off: off + len(data)].tobytes() == data


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_window_refill_edges_at_every_alignment(dev, shift):
    """payloads of 1022 .. 1026 and 1982 .. 1986 bytes (both sides of the window's first two refill points), the payload's first byte 0 - 3
    bytes past a dword boundary: every (n_in + shift) mod 4, so the last dword of the payload is filled whole and byte by byte"""
    seen = set()
    for payload, text in one.window_edge_streams():
        assert zlib.decompress(payload, -15) == text
        seen.add((len(payload) + shift) % 4)
        # K-INFLATE: a hand-made member, its payload behind the 18 bytes of the header
        member = gz.hand_member(payload, text)
        clause, h_text, h_blocks = hostapi.inflate_bgzf_member(member)
        assert clause == 0 and h_text == text and h_blocks == [0, 1, 0]
        buf, off = _painted(member, 18, shift)
        out, st = dev.inflate_bgzf(buf[off: off + len(member)], [0, len(member)])
        assert bytes(out) == text and (st["blocks_stored"], st["blocks_fixed"], st["blocks_dynamic"]) == (0, 1, 0), (len(payload), shift)
        assert _untouched(buf, off, member), (len(payload), shift)
        # K-GUNZIP: the payload itself
        h_out, h_r, h_st, h_win = hostapi.gunzip_call(payload, 0, b"", 1024)
        assert h_out == text and h_r["final"] == 1
        buf, off = _painted(payload, 0, shift)
        out, r, st, win = dev.inflate_gzip(buf[off: off + len(payload)], 0, None, 1024)
        assert bytes(out) == text and r == h_r and {f: st[f] for f in hipapi.GUNZIP_COUNTERS} == h_st and bytes(win) == h_win, (len(payload), shift)
        assert _untouched(buf, off, payload), (len(payload), shift)
    assert seen == {0, 1, 2, 3}


def test_one_decoder_two_kernels(dev):
    """every member of the CPU test through K-INFLATE (one call, the members one behind the other) and its payload through K-GUNZIP: the
    text and the block counters of the host rule from both"""
    members = one.members()
    want = [hostapi.inflate_member(payload, len(text)) for _, payload, text in members]
    assert all(clause == 0 and made == text for (clause, made, _), (_, _, text) in zip(want, members))
    data = b"".join(gz.wrap(payload, zlib.crc32(text), len(text)) for _, payload, text in members)
    out, st = dev.inflate_bgzf(data, gz.member_offsets(data))
    assert bytes(out) == b"".join(text for _, _, text in members)
    assert [st["blocks_stored"], st["blocks_fixed"], st["blocks_dynamic"]] == [sum(b[i] for _, _, b in want) for i in range(3)]
    for (name, payload, text), (_, _, blocks) in zip(members, want):
        h_out, h_r, h_st, _ = hostapi.gunzip_call(payload, 0, b"", 16384)
        out, r, st, _ = dev.inflate_gzip(payload, 0, None, 16384)
        assert bytes(out) == text == h_out and r == h_r and {f: st[f] for f in hipapi.GUNZIP_COUNTERS} == h_st, name
        assert [st["blocks_stored"], st["blocks_fixed"], st["blocks_dynamic"]] == blocks, name
