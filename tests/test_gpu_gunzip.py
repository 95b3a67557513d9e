"""K-GUNZIP on the device (pf_inflate_gzip through hipapi.Device.inflate_gzip; csrc/pf_gunzip.hip) against zlib byte for byte and against
the host rule (hostapi.gunzip_call, the same stages as lane 0 of 1, which tests/test_gunzip_rule_cpu.py pins against zlib): the text, the
window, the end bit, the CRC register, the counters, and the clause and bit of every refusal.  The streams are gzp_cases' A - G."""
import zlib

import numpy as np
import pytest
import torch

import gz_cases as gz
import gzp_cases as gp

from ploidyfrost_amd import hipapi, hostapi

pytestmark = pytest.mark.gpu
COUNTERS = hipapi.GUNZIP_COUNTERS


@pytest.fixture(scope="module")
def dev():
    d = hipapi.Device(0)
    yield d
    d.close()


def _finish(raw_register: int, n: int) -> int:
    # crc(text) = raw(text) ^ crc(zeros of the same length): the CRC is affine in the text
    return raw_register ^ zlib.crc32(b"\0" * n)


def same_as_host(dev, stream, text, piece, start_bit=0, window=b""):
    """one call on the device and on the host: equal in everything; returns (text, result, stats)"""
    out, r, st, win = dev.inflate_gzip(stream, start_bit, window if window else None, piece)
    h_out, h_r, h_st, h_win = hostapi.gunzip_call(stream, start_bit, window, piece)
    assert bytes(out) == h_out
    assert r == h_r
    assert {f: st[f] for f in COUNTERS} == h_st
    assert bytes(win) == h_win
    if text is not None:
        assert bytes(out) == text and r["final"] == 1 and r["end_bit"] > 8 * len(stream) - 8
        assert _finish(r["crc_raw"], len(text)) == zlib.crc32(text) and r["out_bytes"] == len(text)
        assert bytes(win) == (window + text)[-32768:]
    return bytes(out), r, st


def test_stream_a_in_pieces(dev):
    stream, text = gp.streams()["A"]
    assert len(stream) == 227996
    _, _, st = same_as_host(dev, stream, text, 16384)
    assert st["pieces_live"] >= 8 and st["markers"] > 0 and st["pieces_live"] + st["pieces_dead"] == st["pieces_found"]
    assert (st["blocks_stored"], st["blocks_fixed"], st["blocks_dynamic"]) == (0, 0, 14) and st["bytes_in"] == len(stream)
    same_as_host(dev, stream, text, 0)        # the default stride
    _, _, one = same_as_host(dev, stream, text, 1 << 30)
    assert one["pieces_live"] == 1 and one["markers"] == 0


def test_stream_b_many_pieces_within_a_window(dev):
    stream, text = gp.streams()["B"]
    assert len(stream) == 280307
    _, _, st = same_as_host(dev, stream, text, 1024)
    assert st["pieces_live"] >= 200 and st["markers"] > 0 and (st["blocks_fixed"], st["blocks_dynamic"]) == (1, 1806)
    same_as_host(dev, stream, text, 64)


def test_stream_c_far_matches_across_pieces(dev):
    """the 200 random bytes recur at distance 32 400 only, so the stream is shorter than that of the text without the repeats only if
    they are matches of that distance; with pieces of at most a few KB and more than 10 KB of compressed noise between two copies,
    every such match refers to another piece"""
    stream, text = gp.streams()["C"]
    assert len(stream) + 800 < len(gp.raw(gp.text_c(False), 9, 4))
    _, _, st = same_as_host(dev, stream, text, 1024)
    assert st["markers"] > 0 and st["pieces_live"] >= 16
    assert len(stream) / st["pieces_live"] < 5000


@pytest.mark.parametrize("name", ["D_flush", "D_block"])
def test_stream_d_flushes_and_block_ends(dev, name):
    stream, text = gp.streams()[name]
    _, _, st = same_as_host(dev, stream, text, 1024)
    assert st["pieces_live"] >= 50 and (st["blocks_stored"] >= 80) == (name == "D_flush")
    same_as_host(dev, stream, text, 16384)


@pytest.mark.parametrize("name", ["E_stored", "E_fixed"])
def test_stream_e_no_candidate_one_live_piece(dev, name):
    stream, text = gp.streams()[name]
    _, _, st = same_as_host(dev, stream, text, 1024)
    assert st["pieces_live"] == 1 and st["markers"] == 0


def test_stream_f_every_setting_on_every_text(dev):
    names = [n for n in gp.streams() if n.startswith("F_")]
    assert len(names) == len(gz.SETTINGS) * len(gz.texts())
    for i, name in enumerate(names):
        stream, text = gp.streams()[name]
        same_as_host(dev, stream, text, (1024, 64, 16384)[i % 3])


def test_members_of_files_g_call_by_call(dev):
    """the files of G through the container on the host and one device call per member"""
    for name, (data, text) in gp.files().items():
        at, got = 0, b""
        while at < len(data):
            clause, hl = hostapi.gunzip_header(data[at:])
            assert clause == 0, name
            out, r, _ = same_as_host(dev, data[at + hl:], None, 1024)
            assert r["final"] == 1
            end = at + hl + (r["end_bit"] + 7) // 8
            assert data[end: end + 8] == gp.trailer(out)
            got += out
            at = end + 8
        assert got == text, name


def test_cut_in_mid_block_and_carried_on(dev):
    """stream A cut at 20 places: the call returns the last complete block boundary, and the next call, from that bit with the window
    the first one left, completes the text"""
    stream, text = gp.streams()["A"]
    for i in range(20):
        cut = 1000 + i * 11300 + i
        out1, r1, _ = same_as_host(dev, stream[:cut], None, 4096)
        assert r1["final"] == 0 and r1["end_bit"] <= 8 * cut and text.startswith(out1)
        assert (r1["out_bytes"] == 0) == (r1["end_bit"] == 0)
        win = out1[-32768:]
        skip = r1["end_bit"] // 8
        out2, r2, _ = same_as_host(dev, stream[skip:], None, 4096, r1["end_bit"] % 8, win)
        assert out1 + out2 == text and r2["final"] == 1
        n1, n2 = len(out1), len(out2)
        whole = _finish(r1["crc_raw"], n1) if n2 == 0 else None
        # the two registers combined as the stream loop combines them: crc(a + b) = crc(a + zeros) ^ raw(b)
        both = zlib.crc32(out1 + b"\0" * n2) ^ r2["crc_raw"]
        assert both == zlib.crc32(text) and (whole is None or whole == zlib.crc32(text))


def test_every_stream_clause_as_the_host_rule(dev):
    prefix, ptext = gp.sound_prefix()
    for name, bad in gp.stream_refusals().items():
        for stream in (bad, prefix + bad):
            h = hostapi.gunzip_call(stream, 0, b"", 1024)[1]
            if name == "dist_before" and stream is not bad:
                assert h["clause"] == 0     # behind other text the distance is met
                continue
            assert h["clause"] == gp.CLAUSE[name] and h["clause_bit"] == (0 if stream is bad else 8 * len(prefix)), name
            with pytest.raises(hipapi.DeviceError) as e:
                dev.inflate_gzip(stream, 0, None, 1024)
            assert e.value.status == hipapi.PF_ERR_ARG and (e.value.clause, e.value.clause_bit) == (h["clause"], h["clause_bit"]), name
            assert str(e.value).endswith("pf_inflate_gzip: bit %d: %s" % (h["clause_bit"], hostapi.gunzip_clause_text(h["clause"]))), name
    # a distance that the window passed in meets, and one it does not
    bad = gp.stream_refusals()["dist_before"]
    out, r, _ = same_as_host(dev, bad, None, 1024, 0, b"G")
    assert out == b"AGAG" and r["final"] == 1
    # behind other text: a block that reaches 30 000 bytes back, with a window of 100 bytes and 9 000 bytes of text in front of it
    b = gz.Bits()
    gz.block_header(b, 1)
    b.code(*gz.FIXED_LIT[257]); b.code(*gz.FIXED_DIST[29]); b.put(30000 - 24577, 13); b.code(*gz.FIXED_LIT[256])
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    head = c.compress(ptext[:9000]) + c.flush(zlib.Z_FULL_FLUSH)
    stream = head + b.bytes()
    for window, refused in ((b"w" * 100, True), (b"w" * 32768, False)):
        h = hostapi.gunzip_call(stream, 0, window, 64)[1]
        assert (h["clause"] == gp.CLAUSE["dist_before"]) == refused
        if refused:
            with pytest.raises(hipapi.DeviceError) as e:
                dev.inflate_gzip(stream, 0, window, 64)
            assert (e.value.clause, e.value.clause_bit) == (h["clause"], h["clause_bit"]) and h["clause_bit"] == 8 * len(head)
        else:
            out, _, _ = same_as_host(dev, stream, None, 64, 0, window)
            assert out == ptext[:9000] + b"www"


def test_out_cap_one_byte_short(dev):
    stream, text = gp.streams()["A"]
    buf = np.full(len(text) + 8, 0xA5, dtype=np.uint8)
    with pytest.raises(hipapi.DeviceError) as e:
        dev.inflate_gzip(stream, out=buf, out_cap=len(text) - 1)
    assert e.value.status == hipapi.PF_ERR_OVERFLOW and e.value.needed == len(text)
    assert (buf == 0xA5).all()
    out, _, _, _ = dev.inflate_gzip(stream, out=buf, out_cap=len(text))
    assert bytes(out) == text and (buf[len(text):] == 0xA5).all()


def test_device_pointers_at_odd_addresses_and_the_timed_launch(dev):
    stream, text = gp.streams()["D_flush"]
    cut = len(stream) // 2
    out1, r1, _ = same_as_host(dev, stream[:cut], None, 4096)
    skip = r1["end_bit"] // 8
    rest = stream[skip:]
    comp = torch.zeros(len(rest) + 3, dtype=torch.uint8, device="cuda")
    comp[3:] = torch.frombuffer(bytearray(rest), dtype=torch.uint8).cuda()
    win = torch.zeros(32768 + 1, dtype=torch.uint8, device="cuda")
    n_win = min(len(out1), 32768)
    win[1: 1 + n_win] = torch.frombuffer(bytearray(out1[-32768:]), dtype=torch.uint8).cuda()
    buf = torch.full((len(text) - len(out1) + 9,), 0xA5, dtype=torch.uint8, device="cuda")
    dev.enable_timing(True)
    try:
        got, r, st, new_win = dev.inflate_gzip(comp[3:], r1["end_bit"] % 8, win[1: 1 + n_win], 4096, out=buf[1:], out_cap=len(text) - len(out1),
                                               new_window=win[1:])   # (the new window over the old one)
        ms, launches = dev.kernel_time(hipapi.K_GUNZIP)
        assert launches == 1 and ms > 0 and dev.kernel_units(hipapi.K_GUNZIP) == len(text) - len(out1)
        assert all(st["stage_ms"][s] > 0 for s in hipapi.GUNZIP_STAGES)
    finally:
        dev.enable_timing(False)
    host = buf.cpu().numpy()
    n2 = len(text) - len(out1)
    assert out1 + bytes(host[1: 1 + n2]) == text and host[0] == 0xA5 and (host[1 + n2:] == 0xA5).all()
    assert r["final"] == 1 and bytes(win[1:].cpu().numpy()) == text[-32768:]
    h = hostapi.gunzip_call(rest, r1["end_bit"] % 8, out1[-32768:], 4096)
    assert r == h[1] and {f: st[f] for f in COUNTERS} == h[2]


def test_nothing_to_do(dev):
    out, r, st, win = dev.inflate_gzip(b"", 0, None, 0)
    assert len(out) == 0 and r["final"] == 0 and r["end_bit"] == 0 and st["pieces_live"] == 1 and len(win) == 0
    # an empty member: one final block of no bytes
    out, r, st, _ = dev.inflate_gzip(gp.raw(b""), 0, None, 0)
    assert len(out) == 0 and r["final"] == 1 and r["crc_raw"] == 0
