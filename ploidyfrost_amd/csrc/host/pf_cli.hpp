// The idiom of the reads sub-commands' command lines (pf_cli_reads.cpp, pf_cli_build.cpp, pf_cli_run.cpp): every sub-command walks
// argv once, word by word; a word is offered to the option groups below -- take(): 1 = taken (i stands on its last word), 0 = not
// one of the group's, -1 = refused with `why` -- and then to the sub-command's own lines; the first word that offends is refused by
// name with the usage behind it; what can only be judged behind the last word is judged by finish().  A new option that several
// sub-commands take goes into one group; one that a single sub-command takes goes into that sub-command's loop.  What every line
// says is pinned by tests/golden/cli/surface.json.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "pf_count_host.hpp"
#include "pf_trim_host.hpp"
#include "../pf_trim_rule.hpp"

namespace pfcli {
using std::string;
using std::vector;

// `Error: <sub>: <why>` and the sub-command's usage on stderr; the exit status of a refusal
struct Refuse {
    const char *sub, *usage;
    int operator()(const string &why) const { std::cerr << "Error: " << sub << ": " << why << std::endl << usage << std::endl; return 1; }
};

// what the host layer refused, as every sub-command says it
inline int failed(const string &err) { std::cerr << "Error: " << err << std::endl; return 1; }

// the value of the option argv[i] (i moves onto it); null, with `why`, when argv ends behind the option
inline const char *value_of(int argc, char **argv, int &i, string &why) {
    if (i + 1 >= argc) { why = string(argv[i]) + " needs a value"; return nullptr; }
    return argv[++i];
}

// ---- the two number grammars and the reals ----
// digits from the first character to the last: 0 = a number, 1 = not one, 2 = one that does not fit 64 bits
inline int digits(const char *text, uint64_t &v) {
    char *end = nullptr;
    errno = 0;
    v = strtoull(text, &end, 10);
    if (!isdigit((unsigned char)text[0]) || *end) return 1;
    return errno ? 2 : 0;
}
inline bool number(const string &opt, const char *text, uint64_t &v, bool positive, string &why) {
    if (digits(text, v) == 0 && (v > 0 || !positive)) return true;
    why = opt + " takes a " + (positive ? "positive " : "") + "number, not '" + text + "'";
    return false;
}
// a signed number as the C library reads one (blanks and a sign in front), within [0, top]
inline bool ranged(const string &opt, const char *text, long long top, long long &v, string &why) {
    char *end = nullptr;
    errno = 0;
    v = strtoll(text, &end, 10);
    if (!errno && end != text && !*end && v >= 0 && v <= top) return true;
    why = opt + " takes a number from 0 to " + std::to_string(top) + ", not '" + text + "'";
    return false;
}
inline bool real(const string &opt, const char *text, double &v, string &why) {
    char *end = nullptr;
    v = strtod(text, &end);
    if (end != text && !*end && std::isfinite(v)) return true;
    why = opt + " takes a number, not '" + text + "'";
    return false;
}

// ---- kmc's letters of `count`, `mask -k`, `smudge -k`, `run` and `run-multi`, with a detached or an attached value (-k 25, -k25,
// -ci1, -cs10000), and -b ----
struct CountArgs {
    pfh::CountOptions opt;
    string seen;   // the first of -ci -cx -cs -b that was given ("" = none)
    bool k_seen = false;
    int take(int argc, char **argv, int &i, string &why) {
        const string a = argv[i];
        if (a == "-b") { opt.both_strands = false; if (seen.empty()) seen = "-b"; return 1; }
        string name;
        for (const char *o : {"-ci", "-cx", "-cs", "-k"})
            if (a.compare(0, strlen(o), o) == 0 && (a.size() == strlen(o) || isdigit((unsigned char)a[strlen(o)]))) { name = o; break; }
        if (name.empty()) return 0;
        string text = a.substr(name.size());
        if (text.empty()) {
            if (i + 1 >= argc) { why = name + " needs a value"; return -1; }
            text = argv[++i];
        }
        uint64_t v = 0;
        const int bad = digits(text.c_str(), v);
        if (bad == 1) { why = name + " takes a number, not '" + text + "'"; return -1; }
        if (bad == 2) v = pf_count::COUNTER_MAX + 1;   // (refused with the cut-offs, by name)
        if (name == "-k") { opt.k = (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull); k_seen = true; return 1; }
        (name == "-ci" ? opt.ci : name == "-cx" ? opt.cx : opt.cs) = v;
        if (seen.empty()) seen = name;
        return 1;
    }
};

// ---- the reads options: -v and, where the sub-command has them, --gz / --gz-plain, --fasta, --chunk-bytes N, --initial-slots N.  A
// sub-command that refuses one of them by name, or words it in its own way, has its own line for it ----
struct ReadsCli {
    enum { GZ = 1, FASTA = 2, CHUNK = 4, SLOTS = 8, ALL = 15 };
    int has;   // which of the four the sub-command takes
    int gz = 0;
    bool fasta = false, verbose = false;
    uint64_t chunk_bytes = 0, initial_slots = 0;
    explicit ReadsCli(int has_) : has(has_) {}
    int take(int argc, char **argv, int &i, string &why) {
        const string a = argv[i];
        if (a == "-v") { verbose = true; return 1; }
        if ((has & GZ) && a == "--gz") { gz = std::max(gz, 1); return 1; }
        if ((has & GZ) && a == "--gz-plain") { gz = 2; return 1; }
        if ((has & FASTA) && a == "--fasta") { fasta = true; return 1; }
        if (!((has & CHUNK) && a == "--chunk-bytes") && !((has & SLOTS) && a == "--initial-slots")) return 0;
        const char *val = value_of(argc, argv, i, why);
        return val && number(a, val, a == "--chunk-bytes" ? chunk_bytes : initial_slots, true, why) ? 1 : -1;
    }
};

// ---- --phred 33|64 of `qc`, `trim` and the trim words of `run` / `run-multi` ----
struct PhredCli {
    uint32_t phred = 33;
    bool seen = false;
    int take(int argc, char **argv, int &i, string &why) {
        if (strcmp(argv[i], "--phred") != 0) return 0;
        const char *val = value_of(argc, argv, i, why);
        if (!val) return -1;
        if (strcmp(val, "33") != 0 && strcmp(val, "64") != 0) { why = string("--phred takes 33 or 64, not '") + val + "'"; return -1; }
        phred = (uint32_t)atoi(val);
        seen = true;
        return 1;
    }
};

// ---- `--adapters FILE [--adapter-seed S] [--adapter-score T] [--adapter-pairs [--adapter-pair-score T] [--adapter-pair-min A]
// [--adapter-keep-both]]` of `trim`, `run` and `run-multi` ----
struct ClipCli {
    string adapters, seed, score, pair_score, pair_min;
    bool adapters_seen = false, seed_seen = false, score_seen = false, pairs_seen = false, pair_score_seen = false, pair_min_seen = false, keep_both_seen = false;
    int take(int argc, char **argv, int &i, string &why) {
        const string a = argv[i];
        if (a == "--adapter-pairs") { pairs_seen = true; return 1; }
        if (a == "--adapter-keep-both") { keep_both_seen = true; return 1; }
        if (a != "--adapters" && a != "--adapter-seed" && a != "--adapter-score" && a != "--adapter-pair-score" && a != "--adapter-pair-min") return 0;
        const char *v = value_of(argc, argv, i, why);
        if (!v) return -1;
        if (a == "--adapters") { adapters = v; adapters_seen = true; }
        else if (a == "--adapter-seed") { seed = v; seed_seen = true; }
        else if (a == "--adapter-pair-score") { pair_score = v; pair_score_seen = true; }
        else if (a == "--adapter-pair-min") { pair_min = v; pair_min_seen = true; }
        else { score = v; score_seen = true; }
        return 1;
    }
    static bool number(const string &v, uint32_t lo, uint32_t hi, uint32_t &out) {
        if (v.empty() || v.size() > 6) return false;
        for (char ch : v) if (ch < '0' || ch > '9') return false;
        out = (uint32_t)stoul(v);
        return out >= lo && out <= hi;
    }
    // after the last argument: "" = accepted
    string finish(pfh::ClipOptions &opt) const {
        if (!adapters_seen) {
            if (seed_seen) return "--adapter-seed needs --adapters: the seed is read by the adapter clipping alone";
            if (score_seen) return "--adapter-score needs --adapters: the score is read by the adapter clipping alone";
            if (pairs_seen) return "--adapter-pairs needs --adapters: the prefix pairs are read from the adapter file";
            if (pair_score_seen) return "--adapter-pair-score needs --adapters and --adapter-pairs";
            if (pair_min_seen) return "--adapter-pair-min needs --adapters and --adapter-pairs";
            if (keep_both_seen) return "--adapter-keep-both needs --adapters and --adapter-pairs";
            return "";
        }
        if (adapters.empty()) return "--adapters takes the path of a FASTA file";
        opt.adapters = adapters;
        if (seed_seen && !number(seed, 0, pf_clip::MAX_SEED, opt.seed)) return "--adapter-seed takes 0 to 8, not '" + seed + "'";
        if (score_seen && !number(score, pf_clip::MIN_SCORE, pf_clip::MAX_SCORE, opt.score)) return "--adapter-score takes 1 to 1000, not '" + score + "'";
        if (!pairs_seen) {
            if (pair_score_seen) return "--adapter-pair-score needs --adapter-pairs: the score is read by the palindrome mode alone";
            if (pair_min_seen) return "--adapter-pair-min needs --adapter-pairs: the length is read by the palindrome mode alone";
            if (keep_both_seen) return "--adapter-keep-both needs --adapter-pairs: the reverse read is dropped by the palindrome mode alone";
            return "";
        }
        opt.pairs = true;
        opt.keep_both = keep_both_seen;
        if (pair_score_seen && !number(pair_score, pf_clip::MIN_SCORE, pf_clip::MAX_SCORE, opt.pair_score))
            return "--adapter-pair-score takes 1 to 1000, not '" + pair_score + "'";
        if (pair_min_seen && !number(pair_min, pf_clip::MIN_PAIR_MIN, pf_clip::MAX_PAIR_MIN, opt.pair_min))
            return "--adapter-pair-min takes 1 to 16, not '" + pair_min + "'";
        return "";
    }
};

// ---- `--dedup [--dedup-bases N] [--dedup-initial-slots N]` of trim, run and run-multi (K-DEDUP) ----
struct DedupCli {
    string bases, slots;
    bool seen = false, bases_seen = false, slots_seen = false;
    int take(int argc, char **argv, int &i, string &why) {
        const string a = argv[i];
        if (a == "--dedup") { seen = true; return 1; }
        if (a != "--dedup-bases" && a != "--dedup-initial-slots") return 0;
        const char *v = value_of(argc, argv, i, why);
        if (!v) return -1;
        if (a == "--dedup-bases") { bases = v; bases_seen = true; }
        else { slots = v; slots_seen = true; }
        return 1;
    }
    // after the last argument: "" = accepted
    string finish(pfh::DedupOptions &opt) const {
        if (!seen) {
            if (bases_seen) return "--dedup-bases needs --dedup: the bases are read by the duplicate removal alone";
            if (slots_seen) return "--dedup-initial-slots needs --dedup: the table is the duplicate removal's alone";
            return "";
        }
        opt.on = true;
        if (bases_seen && !ClipCli::number(bases, pf_dedup::MIN_BASES, pf_dedup::MAX_BASES, opt.bases)) return "--dedup-bases takes 16 to 4096, not '" + bases + "'";
        if (slots_seen) {
            if (slots.empty() || slots.size() > 12) return "--dedup-initial-slots takes a number of slots up to 2^36, not '" + slots + "'";
            for (char ch : slots) if (ch < '0' || ch > '9') return "--dedup-initial-slots takes a number of slots up to 2^36, not '" + slots + "'";
            opt.initial_slots = stoull(slots);
            if (opt.initial_slots > (1ull << 36)) return "--dedup-initial-slots takes a number of slots up to 2^36, not '" + slots + "'";
        }
        return "";
    }
};

// ---- `run STEP...` / `run-multi STEP...`: the words and options of step 1 as `trim` takes them -- the same refusals and texts ----
struct TrimCli {
    vector<string> words;   // the positional words: the steps
    bool pair_seen = false;
    PhredCli phred;
    string pending1;        // a -1 whose -2 has not come yet
    ClipCli clip;           // --adapters and what goes with it
    DedupCli dedup;         // --dedup and what goes with it
    int take(int argc, char **argv, int &i, const char *sub, vector<string> &files, string &why) {
        const string a = argv[i];
        if (a.empty() || a[0] != '-') { words.push_back(a); return 1; }
        for (const char *o : {"--trimlog", "-o1", "-u1", "-o2", "-u2"})
            if (a == o) { why = a + " is not built into " + sub + ": `trim` writes the trimmed reads, the unpaired ones and the log"; return -1; }
        if (const int taken = clip.take(argc, argv, i, why)) return taken;
        if (const int taken = dedup.take(argc, argv, i, why)) return taken;
        if (const int taken = phred.take(argc, argv, i, why)) return taken;
        if (a != "-1" && a != "-2") return 0;
        const char *v = value_of(argc, argv, i, why);
        if (!v) return -1;
        if (a == "-1") {
            if (!pending1.empty()) { why = no_second(); return -1; }
            pending1 = v;
            pair_seen = true;
        } else {
            if (pending1.empty()) { why = string("-2 ") + v + " has no -1 in front of it (the files of a pair come as -1 <r1.fq> -2 <r2.fq>)"; return -1; }
            files.push_back(pending1);
            files.push_back(v);
            pending1.clear();
        }
        return 1;
    }
    string no_second() const { return "-1 " + pending1 + " has no -2 behind it (the files of a pair come as -1 <r1.fq> -2 <r2.fq>)"; }
    // after the last argument: "" = accepted, with the steps parsed
    string finish(const char *sub, vector<pf_trim_step> &steps, pfh::ClipOptions &clip_opt, pfh::DedupOptions &dedup_opt) const {
        if (!pending1.empty()) return no_second();
        { const string why = clip.finish(clip_opt); if (!why.empty()) return why; }
        { const string why = dedup.finish(dedup_opt); if (!why.empty()) return why; }
        if (words.empty() && (clip_opt.on() || dedup_opt.on)) return "";   // --adapters and --dedup turn trimming on as a step does
        if (words.empty()) {
            if (pair_seen) return string("-1 / -2 need a step: the files of a pair are trimmed together (two files without trimming go with -i: ") + sub + " -i r1.fq -i r2.fq)";
            if (phred.seen) return "--phred needs a step: the quality offset is read by the trimming alone";
            return "";
        }
        vector<const char *> w;
        for (const string &x : words) w.push_back(x.c_str());
        vector<pf_trim::Step> parsed;
        size_t bad = 0;
        const int c = pf_trim::parse_steps(w.data(), w.size(), parsed, &bad);
        if (c) return words[bad] + ": " + pf_trim::refusal_text(c);
        for (const pf_trim::Step &st : parsed) steps.push_back(pf_trim_step{st.kind, st.a, st.b});
        return "";
    }
};
}  // namespace pfcli
