// The reads stream (host/pf_reads_stream.cpp, host/pf_gz_host.cpp) without a device: the few pf_* calls the two files make are stubbed
// below (pinned memory fails, device memory is malloc, a copy is memcpy, the two inflate calls run the rule headers' host decoders), and
// the step is host code -- pf_mask::index_fastq / pf_fasta::index_fasta on the chunk.  What is expected comes from the same rule run
// once over each whole file, never from the stream.  Built with -fsanitize=address,undefined and, where there is one, =thread
// (tests/test_reads_stream_cpu.py).  argv[1]: a directory to write in; it holds gz_text.fq, gz_text.fq.bgz, gz_text.fq.gz and mate.fq.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host/pf_reads_stream.hpp"
#include "pf_fasta_rule.hpp"
#include "pf_gunzip_rule.hpp"
#include "pf_inflate_rule.hpp"
#include "pf_mask_rule.hpp"

// ---- the device, stubbed ----
static std::string g_last_error;
extern "C" {
int pf_host_alloc(pf_ctx *, size_t, void **) { return PF_ERR_HIP; }   // (the pageable path runs)
void pf_host_free(pf_ctx *, void *) { abort(); }
int pf_device_alloc(pf_ctx *, size_t bytes, void **out) { *out = malloc(bytes ? bytes : 1); return *out ? PF_OK : PF_ERR_HIP; }
void pf_device_free(pf_ctx *, void *p) { free(p); }
int pf_copy(pf_ctx *, void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return PF_OK; }
int pf_copy_to_host(pf_ctx *, void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return PF_OK; }
const char *pf_last_error(const pf_ctx *) { return g_last_error.c_str(); }
int pf_inflate_bgzf(pf_ctx *, const uint8_t *comp, uint64_t, const uint64_t *member_off, uint64_t n_members, char *out, uint64_t out_cap, uint64_t *out_bytes,
                    pf_inflate_stats *, uint64_t *bad_member) {
    std::vector<uint8_t> text(65536);
    uint64_t at = 0;
    for (uint64_t m = 0; m < n_members; ++m) {
        uint32_t len = 0;
        const int clause = pf_inflate::inflate_bgzf_member(comp + member_off[m], member_off[m + 1] - member_off[m], text.data(), &len);
        if (clause) {
            g_last_error = "pf_inflate_bgzf: member " + std::to_string(m) + " of the call: " + pf_inflate::clause_text(clause);
            *bad_member = m;
            return PF_ERR_ARG;
        }
        if (at + len > out_cap) return PF_ERR_OVERFLOW;
        memcpy(out + at, text.data(), len);
        at += len;
    }
    *out_bytes = at;
    return PF_OK;
}
int pf_inflate_gzip(pf_ctx *, const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window, uint32_t piece_bytes, char *out,
                    uint64_t out_cap, uint8_t *new_window, pf_gunzip_result *res, pf_gunzip_stats *) {
    std::vector<uint8_t> text, win(pf_gunzip::RING);   // (new_window may be window: the call below may not write over what it reads)
    pf_gunzip::Call r;
    pf_gunzip::inflate_call(comp, n_bytes, start_bit, window, n_window, piece_bytes, text, win.data(), r);
    *res = pf_gunzip_result{r.out_bytes, r.end_bit, r.final, r.n_window, r.crc_raw, r.clause, r.clause_bit};
    if (r.clause) { g_last_error = std::string("pf_inflate_gzip: ") + pf_gunzip::clause_text((int)r.clause); return PF_ERR_ARG; }
    if (r.out_bytes > out_cap) return PF_ERR_OVERFLOW;
    memcpy(out, text.data(), text.size());
    memcpy(new_window, win.data(), r.n_window);
    return PF_OK;
}
}

using namespace pfh;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            fprintf(stderr, "%s:%d: %s fails (err: %s)\n", __FILE__, __LINE__, #cond, g_err.c_str()); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

static std::string g_dir, g_err;
static const uint64_t CHUNKS[] = {1, 7, 4096, 0};

static std::string put(const std::string &name, const std::string &data) {
    const std::string p = g_dir + "/" + name;
    std::ofstream(p, std::ios::binary).write(data.data(), (std::streamsize)data.size());
    return p;
}
static std::string slurp(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}
// record j of input f, `len` bases: the header says which it is
static std::string record(int f, int j, int len, bool newline = true) {
    std::string seq, qual;
    for (int i = 0; i < len; ++i) { seq += "ACGT"[(i * 7 + j + f) & 3]; qual += (char)('#' + (i + j) % 40); }
    return "@f" + std::to_string(f) + "_" + std::to_string(j) + "\n" + seq + "\n+\n" + qual + (newline ? "\n" : "");
}
static std::string fastq_file(int f, int n, int len0, int step, int mod, bool last_newline = true) {
    std::string t;
    for (int j = 0; j < n; ++j) t += record(f, j, len0 + (j % mod) * step, last_newline || j + 1 < n);
    return t;
}
static std::string fasta_file(int f, int n) {
    std::string t;
    for (int j = 0; j < n; ++j) {
        t += ">f" + std::to_string(f) + "_" + std::to_string(j) + " contig\n";
        for (int line = 0; line < 1 + j % 4; ++line) t += std::string((size_t)(40 + (j * 13 + line) % 30), "ACGT"[(j + line) & 3]) + "\n";
    }
    return t;
}
// the rule once over a whole file, un-chunked: what the stream's sums are held to
static uint64_t whole_records(const std::string &text, bool fasta = false) {
    if (fasta) {
        pf_fasta::Index ix;
        CHECK(pf_fasta::index_fasta(text.data(), text.size(), true, ix) == 0 && ix.bytes_used == text.size());
        return ix.n_records;
    }
    uint64_t used = 0, recs = 0, bad = 0;
    CHECK(pf_mask::index_fastq(text.data(), text.size(), true, used, recs, bad) == 0 && used == text.size());
    return recs;
}
static std::vector<ReadsInput> preflight(const std::vector<std::string> &paths, int gz = 0, bool fasta = false) {
    std::vector<ReadsInput> in;
    CHECK(fastq_preflight("t", "read", paths, {g_dir + "/out"}, ReadsOptions{gz, fasta}, in, g_err) == 0 && in.size() == paths.size());
    return in;
}

// ---- the step: the rule on the chunk, as the device calls run it ----
struct Seen {
    uint64_t chunks = 0, reads = 0, used = 0;
    std::vector<uint64_t> per_input = std::vector<uint64_t>(10, 0);   // records of input f, by the headers
    std::vector<int> fasta_of = std::vector<int>(10, -1);             // Chunk::fasta of input f's chunks: 0, 1, or 2 = both seen
    std::string on_device;                                            // one letter per chunk: 'd' device, 'h' host
};
static int index_chunk(const char *text, uint64_t n, bool final, bool fasta, uint64_t &used, uint64_t &reads, uint64_t &bad) {
    int clause;
    if (fasta) {
        pf_fasta::Index ix;
        clause = pf_fasta::index_fasta(text, n, final, ix);
        used = ix.bytes_used;
        reads = ix.n_records;
        bad = 0;
        if (clause) g_last_error = std::string("pf_count_fasta: record 0 of the chunk: ") + pf_fasta::clause_text(clause);
    } else {
        clause = pf_mask::index_fastq(text, n, final, used, reads, bad);
        if (clause) g_last_error = "pf_mask_fastq: record " + std::to_string(bad) + " of the chunk: " + pf_mask::clause_text(clause);
    }
    return clause ? (int)PF_ERR_ARG : (int)PF_OK;
}
// identity: what was used goes out as it is.  keep_even: the records with an odd number in their header are dropped (out_len < used)
static ChunkStep step_of(Seen &s, bool numbered, bool keep_even = false) {
    return [&s, numbered, keep_even](const Chunk &c, Taken &t) {
        ++s.chunks;
        s.on_device += c.on_device ? 'd' : 'h';
        const int rc = index_chunk(c.text, c.n, c.final, c.fasta, t.used, t.reads, t.bad);
        if (rc != PF_OK) return rc;
        s.reads += t.reads;
        s.used += t.used;
        for (uint64_t at = 0; numbered && at < t.used;) {   // every record start: "@f<input>_<number>" (FASTA: '>')
            const char *p = c.text + at;
            const int f = p[2] - '0';
            const uint64_t j = strtoull(p + 4, nullptr, 10);
            if ((p[0] != '@' && p[0] != '>') || p[1] != 'f' || f < 0 || f > 9 || j != s.per_input[(size_t)f]) { g_last_error = "the test's step: a record out of order"; return (int)PF_ERR_HIP; }
            ++s.per_input[(size_t)f];
            if (at == 0) s.fasta_of[(size_t)f] = s.fasta_of[(size_t)f] < 0 || s.fasta_of[(size_t)f] == (int)c.fasta ? (int)c.fasta : 2;
            uint64_t end = at;   // the record's end: the next record start, or the end of what was used
            if (c.fasta) {
                const void *nx = memmem(p + 1, t.used - at - 1, "\n>", 2);
                end = nx ? (uint64_t)(static_cast<const char *>(nx) - c.text) + 1 : t.used;
            } else {
                for (int line = 0; line < 4 && end < t.used; ++line) {
                    const void *nl = memchr(c.text + end, '\n', t.used - end);
                    end = nl ? (uint64_t)(static_cast<const char *>(nl) - c.text) + 1 : t.used;
                }
            }
            if (c.out && (!keep_even || j % 2 == 0)) { memcpy(c.out + t.out_len, p, end - at); t.out_len += end - at; }
            at = end;
        }
        if (!numbered && c.out) { memcpy(c.out, c.text, t.used); t.out_len = t.used; }
        return (int)PF_OK;
    };
}
// the inputs through the step into a file; returns what was written
static std::string stream_to_file(const std::vector<ReadsInput> &in, uint64_t chunk, const ChunkStep &step, int want_rc = 0) {
    const std::string out = g_dir + "/out";
    const int fd = open(out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    CHECK(fd >= 0);
    StreamTimes tm;
    const int rc = stream_fastq(nullptr, "t", in, chunk, fd, out, step, tm, g_err);
    CHECK(close(fd) == 0);
    CHECK(rc == want_rc && (rc != 0) == !g_err.empty());
    return slurp(out);
}

// 1, 2, 3: text files of records with different lengths; an empty file and a one-record file; a carry that outgrows the room in front
static void case_text(const std::vector<std::string> &texts, const std::vector<uint64_t> &chunks) {
    std::vector<std::string> paths;
    std::string all;
    uint64_t total = 0;
    for (size_t f = 0; f < texts.size(); ++f) { paths.push_back(put("in" + std::to_string(f) + ".fq", texts[f])); all += texts[f]; total += whole_records(texts[f]); }
    const std::vector<ReadsInput> in = preflight(paths);
    for (size_t f = 0; f < texts.size(); ++f) CHECK(in[f].path == paths[f] && in[f].size == texts[f].size() && in[f].kind == GZ_KIND_TEXT && !in[f].fasta);
    for (uint64_t chunk : chunks) {
        Seen s;
        CHECK(stream_to_file(in, chunk, step_of(s, true)) == all);
        CHECK(s.reads == total && s.used == all.size() && s.on_device.find('d') == std::string::npos);
        for (size_t f = 0; f < texts.size(); ++f) CHECK(s.per_input[f] == whole_records(texts[f]) && s.fasta_of[f] <= 0);
    }
}

// 4: a malformed record as record 5 of the second input; 11: an input that cannot be read any more once the stream runs
static void case_errors() {
    std::string bad = fastq_file(1, 9, 40, 3, 5);
    const size_t at = bad.find("@f1_4\n");
    bad[bad.find("\n+\n", at) + 1] = 'x';   // the third line of the fifth record
    const std::vector<std::string> paths = {put("e0.fq", fastq_file(0, 12, 30, 7, 4)), put("e1.fq", bad), put("e2.fq", fastq_file(2, 6, 50, 1, 3))};
    const std::vector<ReadsInput> in = preflight(paths);
    for (uint64_t chunk : CHUNKS) {
        Seen s;
        stream_to_file(in, chunk, step_of(s, true), 1);
        CHECK(g_err == "t: " + paths[1] + ": record 5: " + pf_mask::clause_text(pf_mask::CLAUSE_PLUS));
    }
    CHECK(unlink(paths[1].c_str()) == 0 && mkdir(paths[1].c_str(), 0755) == 0);   // (open() takes a directory, read() does not)
    for (uint64_t chunk : CHUNKS) {
        Seen s;
        stream_to_file(in, chunk, step_of(s, true), 1);
        CHECK(g_err == "t: reading " + paths[1] + " (Is a directory)" && s.per_input[0] == 12 && s.per_input[2] == 0);
    }
    PairStreamTimes tm;
    const int rc = stream_fastq_pair(nullptr, "t", in[0], in[1], 512, [](const PairChunk &, PairTaken &) { return (int)PF_OK; }, tm, g_err);
    CHECK(rc == 1 && g_err == "t: reading " + paths[1] + " (Is a directory)");
    CHECK(rmdir(paths[1].c_str()) == 0);
    StreamTimes stm;
    Seen s;
    CHECK(stream_fastq(nullptr, "t", in, 4096, -1, "", step_of(s, true), stm, g_err) == 1 && g_err == "t: cannot read " + paths[1] + " (No such file or directory)");
}

// 5: a step whose output is shorter than its input
static void case_sized() {
    const std::string a = fastq_file(0, 31, 30, 7, 4), b = fastq_file(1, 8, 90, 0, 1, false);
    std::string kept;
    for (int j = 0; j < 31; j += 2) kept += record(0, j, 30 + (j % 4) * 7);
    for (int j = 0; j < 8; j += 2) kept += record(1, j, 90);
    const std::vector<ReadsInput> in = preflight({put("s0.fq", a), put("s1.fq", b)});
    for (uint64_t chunk : CHUNKS) {
        Seen s;
        CHECK(stream_to_file(in, chunk, step_of(s, true, true)) == kept && s.reads == 39);
    }
}

// 6: --fasta: the kind of every chunk by its first byte
static void case_fasta() {
    const std::string fa = fasta_file(0, 90), fq = fastq_file(1, 60, 60, 5, 6);
    CHECK(fa.size() > 2 * 4096 && fq.size() > 2 * 4096);
    const std::vector<std::string> paths = {put("a.fa", fa), put("b.fq", fq)};
    std::vector<ReadsInput> refused;
    CHECK(fastq_preflight("t", "read", paths, {}, ReadsOptions{}, refused, g_err) == 1);
    CHECK(g_err == "t: " + paths[0] + ": record 1: the input is FASTA (first byte '>'): only FASTQ is read");
    const std::vector<ReadsInput> in = preflight(paths, 0, true);
    CHECK(in[0].fasta && in[1].fasta);
    Seen s;
    CHECK(stream_to_file(in, 4096, step_of(s, true)) == fa + fq && s.chunks >= 4);
    CHECK(s.fasta_of[0] == 1 && s.fasta_of[1] == 0 && s.per_input[0] == whole_records(fa, true) && s.per_input[1] == whole_records(fq));
}

// 7: blocked and plain gzip: the text of the plain file, on the device; a text file and a gzip file in one call
static void case_gzip() {
    const std::string text = slurp(g_dir + "/gz_text.fq"), plain = g_dir + "/gz_text.fq";
    const uint64_t recs = whole_records(text);
    CHECK(recs > 0);
    const std::pair<const char *, GzKind> sorts[] = {{"/gz_text.fq.bgz", GZ_KIND_BGZF}, {"/gz_text.fq.gz", GZ_KIND_GZIP}};
    for (const auto &sort : sorts)
        for (int gz = sort.second == GZ_KIND_GZIP ? 2 : 1; gz <= 2; ++gz) {
            const std::vector<ReadsInput> in = preflight({plain, g_dir + sort.first}, gz);
            CHECK(in[0].kind == GZ_KIND_TEXT && in[1].kind == sort.second);
            for (uint64_t chunk : {(uint64_t)4096, (uint64_t)20000}) {
                Seen s;
                CHECK(stream_to_file(in, chunk, step_of(s, false)) == text + text && s.reads == 2 * recs);
                const size_t first_d = s.on_device.find('d');   // the text file's chunks on the host, then the gzip file's on the device
                CHECK(first_d != std::string::npos && first_d > 0 && s.on_device.find('h', first_d) == std::string::npos);
            }
        }
    std::vector<ReadsInput> refused;
    CHECK(fastq_preflight("t", "read", {g_dir + "/gz_text.fq.gz"}, {}, ReadsOptions{1, false}, refused, g_err) == 1 && g_err.find("member 1, byte 0: ") != std::string::npos);
    CHECK(fastq_preflight("t", "read", {g_dir + "/gz_text.fq.bgz"}, {}, ReadsOptions{}, refused, g_err) == 1 && g_err.find("gzip-compressed") != std::string::npos);
}

// ---- pairs ----
// the first `limit` whole records of text[0, n): their bytes and their number
static void take_records(const char *text, uint64_t n, bool final, uint64_t limit, uint64_t &used, uint64_t &recs) {
    used = recs = 0;
    for (uint64_t at = 0; recs < limit;) {
        for (int line = 0; line < 4; ++line) {
            const void *nl = at < n ? memchr(text + at, '\n', n - at) : nullptr;
            if (!nl && !(final && line == 3 && at < n)) return;
            at = nl ? (uint64_t)(static_cast<const char *>(nl) - text) + 1 : n;
        }
        used = at;
        ++recs;
    }
}
struct PairSeen { uint64_t calls = 0, pairs = 0, used[2] = {0, 0}; std::string on_device[2]; };
static PairChunkStep pair_step(PairSeen &s) {
    return [&s](const PairChunk &c, PairTaken &t) {
        ++s.calls;
        uint64_t recs[2], all[2];
        for (int f = 0; f < 2; ++f) take_records(c.text[f], c.n[f], c.final, ~0ull, all[f], recs[f]);
        if (c.final && recs[0] != recs[1]) { g_last_error = "pf_trim_fastq_pair: the files hold different numbers of records"; return (int)PF_ERR_ARG; }
        t.reads = std::min(recs[0], recs[1]);
        for (int f = 0; f < 2; ++f) {
            uint64_t r;
            take_records(c.text[f], c.n[f], c.final, t.reads, t.used[f], r);
            s.used[f] += t.used[f];
            s.on_device[f] += c.on_device[f] ? 'd' : 'h';
        }
        s.pairs += t.reads;
        return (int)PF_OK;
    };
}
// 8, 9, 10
static void case_pairs() {
    const std::string a = fastq_file(0, 200, 30, 5, 7), b = fastq_file(1, 200, 50, 3, 11, false), b_short = fastq_file(1, 150, 50, 3, 11);
    const std::vector<std::string> paths = {put("p1.fq", a), put("p2.fq", b), put("p2_short.fq", b_short)};
    const std::vector<ReadsInput> in = preflight(paths);
    PairStreamTimes tm;
    for (uint64_t chunk : {(uint64_t)512, (uint64_t)0}) {
        PairSeen s;
        CHECK(stream_fastq_pair(nullptr, "t", in[0], in[1], chunk, pair_step(s), tm, g_err) == 0 && g_err.empty());
        CHECK(s.pairs == 200 && s.used[0] == a.size() && s.used[1] == b.size() && (chunk == 0 || s.calls > 10));
    }
    {   // the second file ends after 150 records
        PairSeen s;
        CHECK(stream_fastq_pair(nullptr, "t", in[0], in[2], 512, pair_step(s), tm, g_err) == 1 && s.pairs == 150);
        const std::string head = "t: " + paths[2] + " ends after 150 records while " + paths[0] + " holds more (at least ";
        const std::string tail = "): the files of a pair hold the same number of records";
        CHECK(g_err.compare(0, head.size(), head) == 0 && g_err.size() > head.size() + tail.size() && g_err.compare(g_err.size() - tail.size(), tail.size(), tail) == 0);
        const uint64_t at_least = strtoull(g_err.c_str() + head.size(), nullptr, 10);
        CHECK(at_least > 150 && at_least <= 200);
        PairSeen whole;   // one call holds both files whole: the device call itself sees the counts
        CHECK(stream_fastq_pair(nullptr, "t", in[0], in[2], 0, pair_step(whole), tm, g_err) == 1);
        CHECK(g_err == "t: " + paths[0] + " holds 200 records, " + paths[2] + " holds 150: the files of a pair hold the same number of records");
    }
    {   // a text file with a blocked-gzip file, and with a plain-gzip file
        const std::string mate = slurp(g_dir + "/mate.fq"), text = slurp(g_dir + "/gz_text.fq");
        CHECK(whole_records(mate) == whole_records(text));
        for (const char *name : {"/gz_text.fq.bgz", "/gz_text.fq.gz"}) {
            const std::vector<ReadsInput> mixed = preflight({g_dir + "/mate.fq", g_dir + name}, 2);
            for (uint64_t chunk : {(uint64_t)512, (uint64_t)4096}) {
                PairSeen s;
                CHECK(stream_fastq_pair(nullptr, "t", mixed[0], mixed[1], chunk, pair_step(s), tm, g_err) == 0);
                CHECK(s.pairs == whole_records(text) && s.used[0] == mate.size() && s.used[1] == text.size());
                CHECK(s.on_device[0].find('d') == std::string::npos && s.on_device[1].find('h') == std::string::npos);
            }
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    g_dir = argv[1];
    const std::vector<uint64_t> chunks(CHUNKS, CHUNKS + 4);
    case_text({fastq_file(0, 25, 20, 9, 5), fastq_file(1, 40, 75, 1, 3), fastq_file(2, 17, 33, 4, 8, false)}, chunks);                       // 1
    case_text({fastq_file(0, 9, 40, 2, 3), "", fastq_file(2, 1, 60, 0, 1), fastq_file(3, 5, 25, 6, 2)}, chunks);                             // 2
    case_text({fastq_file(0, 6, 40, 2, 3) + record(0, 6, 70000) + record(0, 7, 45), fastq_file(1, 4, 30, 1, 2)}, {4096});                    // 3
    case_errors();                                                                                                                       // 4, 11
    case_sized();                                                                                                                        // 5
    case_fasta();                                                                                                                        // 6
    case_gzip();                                                                                                                         // 7
    case_pairs();                                                                                                                        // 8, 9, 10
    printf("ok\n");
    return 0;
}
