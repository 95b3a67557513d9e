// What the reads sub-commands (`mask`, `count`, `trim`, `build`, `build-multi`, `run`, `run-multi`) each used to write out for
// themselves: the context that dies with its scope, write() to the end, the device's "record R of the chunk" in the sub-command's
// words, the sum of two trim counts, and outputs that appear under their names only when all of them are whole.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ploidyfrost_hip.h"

namespace pfh {

// destroys the context on the way out; c = nullptr hands it on (`run`, `run-multi`: to the loader of the calling run)
struct CtxGuard {
    pf_ctx *c;
    ~CtxGuard() { if (c) pf_destroy(c); }
};

// all n bytes, whatever write() takes at a time.  false: errno says why
inline bool write_all(int fd, const void *p, uint64_t n) {
    const char *c = static_cast<const char *>(p);
    for (uint64_t done = 0; done < n;) {
        const ssize_t put = write(fd, c + done, (size_t)(n - done));
        if (put < 0 && errno == EINTR) continue;
        if (put < 0) return false;
        done += (uint64_t)put;
    }
    return true;
}
// the same, worded: `who: writing name (why)`
inline bool write_all(int fd, const void *p, uint64_t n, const std::string &who, const std::string &name, std::string &err) {
    if (write_all(fd, p, n)) return true;
    err = who + ": writing " + name + " (" + strerror(errno) + ")";
    return false;
}

// "[file f: ]record R of the chunk: clause" of a device call (`why`, pf_last_error) as a sub-command words it: the input's path and
// the 1-based record from the start of that input
inline std::string reword_record(const std::string &why, const std::string &who, const std::string &path, uint64_t record_1based) {
    const size_t at = why.find("of the chunk: ");
    return at != std::string::npos ? who + ": " + path + ": record " + std::to_string(record_1based) + ": " + why.substr(at + 14) : who + ": " + path + ": " + why;
}

inline void add_trim_stats(pf_trim_stats &a, const pf_trim_stats &b) {
    a.reads += b.reads; a.kept += b.kept; a.dropped += b.dropped; a.bases += b.bases; a.bases_kept += b.bases_kept;
    a.both += b.both; a.only1 += b.only1; a.only2 += b.only2; a.neither += b.neither;
}

// the outputs of a run: written under temporary names, renamed together at the end; nothing is left under any name otherwise
struct OutFiles {
    struct File { std::string path, tmp; int fd = -1; };
    std::string who;   // "trim", "mask": the first word of every refusal
    std::vector<File> f;
    bool committed = false;
    explicit OutFiles(const char *who_) : who(who_) {}
    int open_all(const std::vector<std::string> &paths, std::string &err) {
        for (const std::string &p : paths) {
            File o;
            o.path = p;
            o.tmp = p + ".tmp." + std::to_string((long)getpid());
            o.fd = open(o.tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (o.fd < 0) { err = who + ": cannot write " + o.tmp + " (" + strerror(errno) + ")"; return 1; }
            f.push_back(o);
        }
        return 0;
    }
    int commit(std::string &err) {
        for (File &o : f) {
            const int rc = close(o.fd);
            o.fd = -1;
            if (rc != 0 && err.empty()) err = who + ": closing " + o.tmp + " (" + strerror(errno) + ")";
        }
        for (size_t i = 0; i < f.size() && err.empty(); ++i)
            if (rename(f[i].tmp.c_str(), f[i].path.c_str()) != 0) {
                err = who + ": renaming " + f[i].tmp + " to " + f[i].path + " (" + strerror(errno) + ")";
                for (size_t j = 0; j < i; ++j) unlink(f[j].path.c_str());
            }
        committed = err.empty();
        return committed ? 0 : 1;
    }
    ~OutFiles() {
        if (committed) return;
        for (File &o : f) {
            if (o.fd >= 0) close(o.fd);
            unlink(o.tmp.c_str());
        }
    }
};

}  // namespace pfh
