// Blocked-gzip output (`--gz-out`) for the reads sub-commands that write reads (`trim`, `mask`): the writer threads beside the device
// stage, and the device side of a compressed output.  The rule is ../pf_deflate_rule.hpp, the kernel K-DEFLATE (pf_deflate_bgzf).
#pragma once
#include <stdint.h>

#include <chrono>
#include <memory>
#include <string>
#include <thread>

#include "pf_host_util.hpp"
#include "pf_reads_stream.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

// ---- writers beside the device stage ----
struct WritePiece {
    std::shared_ptr<char> p;
    uint64_t len = 0;
};
struct PieceWriter {   // writes the pieces of one output in order, at most two behind the device stage
    Chan<int> tokens;
    Chan<WritePiece> pieces;
    std::string err;
    double write_s = 0;
    std::thread th;
    void start(int fd, const std::string &who, const std::string &name) {
        tokens.push(0);
        tokens.push(0);
        th = std::thread([this, fd, who, name] {
            WritePiece w;
            while (pieces.pop(w)) {
                const auto t0 = std::chrono::steady_clock::now();
                if (err.empty()) write_all(fd, w.p.get(), w.len, who, name, err);
                write_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                w.p.reset();
                tokens.push(0);
            }
        });
    }
    void put(WritePiece w) {
        int token;
        if (tokens.pop(token)) pieces.push(std::move(w));
    }
    void stop() {
        pieces.close();
        if (th.joinable()) th.join();
        tokens.close();
    }
};
// The device side of one `--gz-out` output (blocked-gzip output, ../pf_deflate_rule.hpp): the step writes its output on the device
// behind the output's carry (place), take() deflates the whole cuts of 65 280 bytes (K-DEFLATE, pf_deflate_bgzf), keeps the remainder
// below 65 280 bytes on the device (a device-to-device copy to the front) and fetches the packed members; the last take deflates the
// remainder as one short member and appends the 28-byte end-of-file marker.  The file is therefore a function of its text alone, and
// the text never crosses PCIe.
struct GzOut {
    pf_ctx *ctx = nullptr;
    char *d_text = nullptr;
    uint8_t *d_comp = nullptr;
    uint64_t text_cap = 0, comp_cap = 0, carry = 0;
    uint64_t text_bytes = 0, file_bytes = 0;   // taken so far, written so far
    explicit GzOut(pf_ctx *c) : ctx(c) {}
    GzOut(const GzOut &) = delete;
    GzOut &operator=(const GzOut &) = delete;
    ~GzOut();
    // device memory for `room` more bytes of output behind the carry.  null: err is worded
    char *place(const std::string &who, uint64_t room, std::string &err);
    // `added` bytes stand behind the carry; last: the output ends with them.  piece[0, *len) = the bytes for the file (none: *len = 0)
    bool take(const std::string &who, uint64_t added, bool last, std::shared_ptr<char> &piece, uint64_t *len, std::string &err);
};

// one `--gz-out` output: the step writes on the device behind the carry (place), take() deflates there (GzOut) and
// hands the packed members to the writer thread; finish() writes the remainder as one short member and the end-of-file marker
struct GzOutFile {
    GzOut gz;
    PieceWriter wr;
    std::string who;
    explicit GzOutFile(pf_ctx *ctx) : gz(ctx) {}
    void start(int fd, const std::string &who_, const std::string &name) { who = who_; wr.start(fd, who, name); }
    char *place(uint64_t room, std::string &err) { return gz.place(who, room, err); }
    bool take(uint64_t added, bool last, std::string &err) {
        WritePiece w;
        if (!gz.take(who, added, last, w.p, &w.len, err)) return false;
        if (w.len) wr.put(std::move(w));
        return true;
    }
    bool finish(std::string &err) { return take(0, true, err); }
    void stop() { wr.stop(); }
};

}  // namespace pfh
