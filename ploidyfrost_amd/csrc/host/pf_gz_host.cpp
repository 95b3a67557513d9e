#include "pf_gz_host.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>

#include "../pf_gunzip_rule.hpp"
#include "../pf_inflate_rule.hpp"

namespace pfh {

namespace {
constexpr uint64_t GZ_READ_STEP = 4u << 20;   // bytes a read() asks for
std::string member_refusal(const std::string &who, const std::string &path, uint64_t member0, uint64_t byte, const std::string &what) {
    return who + ": " + path + ": member " + std::to_string(member0 + 1) + ", byte " + std::to_string(byte) + ": " + what;
}
}  // namespace

bool BlockReader::open_file(const std::string &who_, const std::string &path_, GzKind kind_, std::string &err) {
    close_file();
    who = who_;
    path = path_;
    kind = kind_;
    pos = members = 0;
    ahead.clear();
    fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = who + ": cannot read " + path + " (" + strerror(errno) + ")"; return false; }
    return true;
}
void BlockReader::close_file() {
    if (fd >= 0) close(fd);
    fd = -1;
}

bool BlockReader::next(char *buf, uint64_t cap, uint64_t chunk, FileBlock &b, std::string &err) {
    if (kind == GZ_KIND_BGZF) return next_members(buf, cap, chunk, b, err);
    b = FileBlock{};
    b.file_off = pos;
    const uint64_t want = std::min(cap, block_bytes(kind, chunk));
    while (b.len < want) {
        const ssize_t got = read(fd, buf + b.len, (size_t)(want - b.len));   // (nothing else moves the descriptor: it stands at pos + len)
        if (got < 0 && errno == EINTR) continue;
        if (got < 0) { err = who + ": reading " + path + " (" + strerror(errno) + ")"; return false; }
        if (got == 0) { b.eof = true; break; }
        b.len += (uint64_t)got;
    }
    pos += b.len;
    return true;
}

bool BlockReader::next_members(char *buf, uint64_t cap, uint64_t chunk, FileBlock &b, std::string &err) {
    b = FileBlock{};
    b.file_off = pos;
    b.first_member = members;
    b.member_off.push_back(0);
    uint64_t fill = std::min<uint64_t>(ahead.size(), cap);   // (what the last call read ahead; never more than the same buffer held)
    if (fill) memcpy(buf, ahead.data(), (size_t)fill);
    bool file_end = false;
    for (;;) {
        // bytes of the next member that are not in the buffer yet are read first: a member is at most GZ_MEMBER_MAX bytes
        while (!file_end && fill < cap && fill - b.len < GZ_MEMBER_MAX) {
            const ssize_t got = pread(fd, buf + fill, (size_t)std::min<uint64_t>(cap - fill, GZ_READ_STEP), (off_t)(pos + fill));
            if (got < 0 && errno == EINTR) continue;
            if (got < 0) { err = who + ": reading " + path + " (" + strerror(errno) + ")"; return false; }
            if (got == 0) file_end = true;
            fill += (uint64_t)got;
        }
        const uint64_t avail = fill - b.len;
        if (avail == 0 && file_end) { b.eof = true; break; }
        if (avail < GZ_MEMBER_MAX && !file_end) break;   // the buffer is full
        pf_inflate::Header h;
        const int clause = pf_inflate::parse_member(reinterpret_cast<const uint8_t *>(buf) + b.len, avail, &h);
        if (clause) {   // (avail reaches the end of the file, or holds any member whole: "past the end" is of the file)
            err = member_refusal(who, path, members, pos + b.len, pf_inflate::clause_text(clause));
            return false;
        }
        if (b.member_off.size() > 1 && b.inflated + h.isize > chunk) break;
        b.len += h.member_len;
        b.inflated += h.isize;
        b.member_off.push_back(b.len);
        ++members;
    }
    if (file_end && fill == b.len) b.eof = true;
    ahead.assign(buf + b.len, buf + fill);
    pos += b.len;
    return true;
}

struct GzText::Plain {
    pf_gunzip::Stream stream;
    char *d_win = nullptr;     // the member's last 32 KiB of text
    uint32_t n_window = 0;
};

GzText::GzText(pf_ctx *c) : ctx(c) {}
GzText::~GzText() {
    if (plain) pf_device_free(ctx, plain->d_win);
    pf_device_free(ctx, d_comp);
    pf_device_free(ctx, d_off);
    pf_device_free(ctx, d_text[0]);
    pf_device_free(ctx, d_text[1]);
}

bool GzText::append(const std::string &who, const std::string &path, const char *comp, const FileBlock &b, std::string &err) {
    auto dev_err = [&](const char *what) { err = who + ": " + path + ": " + what + ": " + pf_last_error(ctx); return false; };
    auto room = [&](void **p, uint64_t &cap, uint64_t need) {
        if (need <= cap && *p) return true;
        pf_device_free(ctx, *p);
        *p = nullptr;
        cap = need + need / 8 + 256;
        return pf_device_alloc(ctx, (size_t)cap, p) == PF_OK;
    };
    const uint64_t left = end - begin, n_off = b.member_off.size();
    const int other = cur ^ 1;
    if (!room(reinterpret_cast<void **>(&d_comp), comp_cap, b.len) || !room(reinterpret_cast<void **>(&d_off), off_cap, n_off * 8) ||
        !room(reinterpret_cast<void **>(&d_text[other]), text_cap[other], left + b.inflated + 16))
        return dev_err("device memory for the chunk");
    if (left && pf_copy(ctx, d_text[other], d_text[cur] + begin, (size_t)left) != PF_OK) return dev_err("carrying the cut record");
    if (pf_copy(ctx, d_comp, comp, (size_t)b.len) != PF_OK || pf_copy(ctx, d_off, b.member_off.data(), (size_t)(n_off * 8)) != PF_OK)
        return dev_err("uploading the compressed chunk");
    uint64_t out_bytes = 0, bad = 0;
    const int rc = pf_inflate_bgzf(ctx, reinterpret_cast<const uint8_t *>(d_comp), b.len, d_off, n_off - 1, d_text[other] + left, b.inflated, &out_bytes,
                                   nullptr, &bad);
    if (rc != PF_OK) {
        const std::string why = pf_last_error(ctx);
        const size_t at = why.find("of the call: ");
        if (rc != PF_ERR_ARG || at == std::string::npos || bad + 1 >= n_off) return dev_err("inflating");
        err = member_refusal(who, path, b.first_member + bad, b.file_off + b.member_off[bad], why.substr(at + 13));
        return false;
    }
    cur = other;
    begin = 0;
    end = left + out_bytes;
    return true;
}

bool GzText::append_plain(const std::string &who, const std::string &path, const char *raw, uint64_t len, uint64_t file_off, bool eof, std::string &err) {
    auto dev_err = [&](const char *what) { err = who + ": " + path + ": " + what + ": " + pf_last_error(ctx); return false; };
    if (!plain || file_off == 0) {
        if (plain) pf_device_free(ctx, plain->d_win);
        plain.reset(new Plain);
    }
    Plain &pl = *plain;
    if (!pl.d_win && pf_device_alloc(ctx, pf_gunzip::RING, reinterpret_cast<void **>(&pl.d_win)) != PF_OK) return dev_err("device memory for the window");
    // what is left moves to the front of the other buffer; every call of this turn writes behind it
    const uint64_t left = end - begin;
    const int other = cur ^ 1;
    auto text_room = [&](int t, uint64_t need, uint64_t keep) {   // d_text[t] holds `need` bytes, its first `keep` kept
        if (need <= text_cap[t] && d_text[t]) return true;
        char *grown = nullptr;
        const uint64_t cap = need + need / 4 + 256;
        if (pf_device_alloc(ctx, (size_t)cap, reinterpret_cast<void **>(&grown)) != PF_OK) return false;
        if (keep && pf_copy(ctx, grown, d_text[t], (size_t)keep) != PF_OK) { pf_device_free(ctx, grown); return false; }
        pf_device_free(ctx, d_text[t]);
        d_text[t] = grown;
        text_cap[t] = cap;
        return true;
    };
    if (!text_room(other, left + 5 * (pl.stream.carry.size() + len) + 65536, 0)) return dev_err("device memory for the chunk");
    if (left && pf_copy(ctx, d_text[other], d_text[cur] + begin, (size_t)left) != PF_OK) return dev_err("carrying the cut record");
    cur = other;
    begin = 0;
    end = left;
    auto call = [&](const uint8_t *bytes, uint64_t n, uint64_t start_bit, bool fresh, pf_gunzip::Call &r, std::string &e) {
        if (fresh) pl.n_window = 0;
        if (n > comp_cap || !d_comp) {
            pf_device_free(ctx, d_comp);
            d_comp = nullptr;
            comp_cap = n + n / 8 + 256;
            if (pf_device_alloc(ctx, (size_t)comp_cap, reinterpret_cast<void **>(&d_comp)) != PF_OK) { dev_err("device memory for the chunk"); e = err; return false; }
        }
        if (n && pf_copy(ctx, d_comp, bytes, (size_t)n) != PF_OK) { dev_err("uploading the compressed chunk"); e = err; return false; }
        pf_gunzip_result res = {};
        int rc = PF_OK;
        for (int turn = 0; turn < 3; ++turn) {   // (a text buffer too small is said before anything is written)
            rc = pf_inflate_gzip(ctx, reinterpret_cast<const uint8_t *>(d_comp), n, start_bit, reinterpret_cast<const uint8_t *>(pl.d_win), pl.n_window, 0,
                                 d_text[cur] + end, text_cap[cur] - end, reinterpret_cast<uint8_t *>(pl.d_win), &res, nullptr);
            if (rc != PF_ERR_OVERFLOW) break;
            if (!text_room(cur, end + res.out_bytes + 16, end)) { dev_err("device memory for the chunk"); e = err; return false; }
        }
        if (rc == PF_ERR_ARG && res.clause) { r.clause = res.clause; r.clause_bit = res.clause_bit; return true; }
        if (rc != PF_OK) { dev_err("inflating"); e = err; return false; }
        r.out_bytes = res.out_bytes;
        r.end_bit = res.end_bit;
        r.final = res.final;
        r.n_window = res.n_window;
        r.crc_raw = res.crc_raw;
        pl.n_window = res.n_window;
        end += res.out_bytes;
        return true;
    };
    std::string e;
    if (!pl.stream.feed(reinterpret_cast<const uint8_t *>(raw), len, eof, call, e)) {
        if (pl.stream.clause) err = member_refusal(who, path, pl.stream.member, pl.stream.clause_byte, pf_gunzip::clause_text(pl.stream.clause));
        else if (err.empty()) err = who + ": " + path + ": " + e;
        return false;
    }
    return true;
}

bool GzText::fetch(std::vector<char> &host, std::string &err) const {
    host.resize(size());
    if (size() && pf_copy(ctx, host.data(), text(), (size_t)size()) != PF_OK) { err = std::string("fetching the inflated text: ") + pf_last_error(ctx); return false; }
    return true;
}

}  // namespace pfh
