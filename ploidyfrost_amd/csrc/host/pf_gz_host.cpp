#include "pf_gz_host.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>

#include "../pf_inflate_rule.hpp"

namespace pfh {

namespace {
constexpr uint64_t GZ_READ_STEP = 4u << 20;   // bytes a read() asks for
std::string member_refusal(const std::string &who, const std::string &path, uint64_t member0, uint64_t byte, const std::string &what) {
    return who + ": " + path + ": member " + std::to_string(member0 + 1) + ", byte " + std::to_string(byte) + ": " + what;
}
}  // namespace

bool gz_magic(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    unsigned char m[2];
    const ssize_t got = read(fd, m, 2);
    close(fd);
    return got == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

bool GzReader::open_file(const std::string &who_, const std::string &path_, std::string &err) {
    close_file();
    who = who_;
    path = path_;
    pos = members = 0;
    ahead.clear();
    fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = who + ": cannot read " + path + " (" + strerror(errno) + ")"; return false; }
    return true;
}
void GzReader::close_file() {
    if (fd >= 0) close(fd);
    fd = -1;
}

bool GzReader::next(char *buf, uint64_t cap, uint64_t chunk, GzBlock &b, std::string &err) {
    b = GzBlock{};
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

GzText::~GzText() {
    pf_device_free(ctx, d_comp);
    pf_device_free(ctx, d_off);
    pf_device_free(ctx, d_text[0]);
    pf_device_free(ctx, d_text[1]);
}

bool GzText::append(const std::string &who, const std::string &path, const char *comp, const GzBlock &b, std::string &err) {
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

bool GzText::fetch(std::vector<char> &host, std::string &err) const {
    host.resize(size());
    if (size() && pf_copy(ctx, host.data(), text(), (size_t)size()) != PF_OK) { err = std::string("fetching the inflated text: ") + pf_last_error(ctx); return false; }
    return true;
}

}  // namespace pfh
