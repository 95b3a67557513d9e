#include "pf_gz_out_host.hpp"

#include <cstring>

#include "../pf_deflate_rule.hpp"

namespace pfh {

GzOut::~GzOut() {
    pf_device_free(ctx, d_text);
    pf_device_free(ctx, d_comp);
}

char *GzOut::place(const std::string &who, uint64_t room, std::string &err) {
    const uint64_t need = carry + room + 1;
    if (need > text_cap || !d_text) {
        void *p = nullptr;
        const uint64_t cap = need + need / 8 + pf_deflate::MEMBER_TEXT;
        if (pf_device_alloc(ctx, (size_t)cap, &p) != PF_OK || (carry && pf_copy(ctx, p, d_text, (size_t)carry) != PF_OK)) {
            err = who + ": device memory for the output's text: " + pf_last_error(ctx);
            pf_device_free(ctx, p);
            return nullptr;
        }
        pf_device_free(ctx, d_text);
        d_text = static_cast<char *>(p);
        text_cap = cap;
    }
    return d_text + carry;
}

bool GzOut::take(const std::string &who, uint64_t added, bool last, std::shared_ptr<char> &piece, uint64_t *len, std::string &err) {
    auto dev_err = [&](const char *what) { err = who + ": " + what + ": " + pf_last_error(ctx); return false; };
    *len = 0;
    piece.reset();
    const uint64_t have = carry + added;
    const uint64_t whole = last ? have : have - have % pf_deflate::MEMBER_TEXT;
    const uint64_t bound = pf_deflate::bound(whole, pf_deflate::MEMBER_TEXT), tail = last ? sizeof pf_deflate::EOF_MARKER : 0;
    uint64_t packed = 0;
    if (whole) {
        if (bound > comp_cap || !d_comp) {
            pf_device_free(ctx, d_comp);
            d_comp = nullptr;
            void *p = nullptr;
            if (pf_device_alloc(ctx, (size_t)(bound + bound / 8), &p) != PF_OK) return dev_err("device memory for the members");
            d_comp = static_cast<uint8_t *>(p);
            comp_cap = bound + bound / 8;
        }
        if (pf_deflate_bgzf(ctx, d_text, whole, pf_deflate::MEMBER_TEXT, d_comp, comp_cap, &packed, nullptr, nullptr) != PF_OK) return dev_err("K-DEFLATE");
    }
    if (packed + tail) {
        piece = std::shared_ptr<char>(new char[packed + tail], std::default_delete<char[]>());
        if (packed && pf_copy(ctx, piece.get(), d_comp, (size_t)packed) != PF_OK) return dev_err("fetching the members");
        if (tail) memcpy(piece.get() + packed, pf_deflate::EOF_MARKER, tail);
    }
    carry = have - whole;   // below 65 280 <= whole: the two ranges do not overlap
    if (carry && whole && pf_copy(ctx, d_text, d_text + whole, (size_t)carry) != PF_OK) return dev_err("keeping the output's remainder");
    text_bytes += whole;
    file_bytes += packed + tail;
    *len = packed + tail;
    return true;
}

}  // namespace pfh
