// K-DEDUP: the rule of `--dedup` -- which reads of a stream are duplicates of an earlier one.  Integers only, shared by the host
// restatement (pfh_dedup_key, pfh_dedup_units) and the kernel (pf_dedup.hip).
//
//   unit       a single-ended call: one record; a pair call: record r of both files together.
//   takes part a unit K-TRIM keeps after the clip and every step -- single-ended: its final interval is not empty; a pair: both
//              records are kept.  (A pair of which one record survives alone is no unit and is written untouched.)
//   code       Aa 0, Cc 1, Gg 2, Tt 3, anything else 4: neither case nor which other byte it is distinguishes reads.
//   key        of the RAW sequence line, before clip and trim.  With B = bases (0: the whole read) a read gives its first
//              L = min(n, B or n) bases, cut into words of 16 bases at 3 bits a base (base 16 j + i at bits 3 i of word j).  Word j of
//              read 1 has index j, word j of read 2 index SECOND + j, SECOND = 2^62: the index spaces of the two reads are disjoint for every read a
//              chunk can hold (j < 2^28), so (R1, R2) and (R2, R1) key apart at any length.  x mixes the whole index into the word.
//              Half h of the key is the sum mod 2^64 of term(x, h) over all words of the unit -- any order, so the lanes of a row
//              hash their own 16 bases each and add -- closed by a mix with the lengths: close(sum, L1, L2, pair, h), forced to be
//              non-zero.  (R1, R2) and (R2, R1) differ in their indices.  Two keys, 128 bits: KEY[0], KEY[1].
//   decision   units are numbered in stream order since the dedup was opened; among the units that take part and have one key the one
//              with the smallest number is kept, every other one is dropped (its interval becomes empty in both files, as if MINLEN
//              had dropped it).  A function of the stream alone: chunking, table size, growth and atomic order do not enter.
//   statistics units (taking part), unique (distinct keys), duplicates = units - unique, max_copies, levels[c - 1] = keys with c
//              copies (levels[9]: 10 or more).
//   table      slots of 32 bytes {h1, h2, ~first unit, copies}, a power of two of them, all 0 = empty; the home slot of a key is
//              home(h1, slots), probing is linear.  Before n units are inserted, 2 * (entries + n) <= slots (needed_slots).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PF_DEDUP_HD __host__ __device__
#else
#define PF_DEDUP_HD
#endif

namespace pf_dedup {

constexpr uint32_t MIN_BASES = 16, MAX_BASES = 4096;   // of `bases` when it is not 0
constexpr uint64_t MIN_SLOTS = 64, DEFAULT_SLOTS = 1ull << 20;
constexpr uint32_t WORD_BASES = 16, CODE_BITS = 3, LEVELS = 10;
constexpr uint64_t SECOND = 1ull << 62;                // index of read 2's word 0: beyond every index of read 1 (a chunk's line has fewer than 2^32 bytes: j < 2^28)
constexpr uint64_t SEED1 = 0x9E3779B97F4A7C15ull, SEED2 = 0xD1B54A32D192ED03ull, SEED_LEN = 0x8CB92BA72F3D8DD7ull;

PF_DEDUP_HD inline bool bases_ok(uint32_t bases) { return bases == 0 || (bases >= MIN_BASES && bases <= MAX_BASES); }

PF_DEDUP_HD inline uint64_t mix64(uint64_t x) {   // splitmix64's finalizer
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
PF_DEDUP_HD inline uint32_t code(uint8_t c) {
    c &= 0xDFu;   // (folds the letters' case; no other byte becomes a letter by it)
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
// the bases of a read that enter the key
PF_DEDUP_HD inline uint32_t covered(uint32_t n, uint32_t bases) { return bases && bases < n ? bases : n; }
// the index of word j of read `second`.  term() lays its low 16 bits above the word's 48 and mixes the rest (read 2's bit 62 among
// it) into all 64 bits, so two (word, index) pairs give one x only by a collision of mix64
PF_DEDUP_HD inline uint64_t index_of(uint64_t j, bool second) { return second ? SECOND + j : j; }
PF_DEDUP_HD inline uint64_t term(uint64_t word, uint64_t index, int half) {
    const uint64_t x = word ^ (index << 48) ^ mix64(index >> 16);   // read 1, index < 2^16: word | index << 48
    return half == 0 ? mix64(x ^ SEED1) : mix64(mix64(x + SEED2) ^ x);
}
PF_DEDUP_HD inline uint64_t close(uint64_t sum, uint32_t l1, uint32_t l2, bool pair, int half) {
    const uint64_t lens = (uint64_t)l1 | ((uint64_t)l2 << 32);
    const uint64_t h = mix64(sum ^ mix64(lens + SEED_LEN * (uint64_t)(2 * half + (pair ? 1 : 0) + 1)));
    return h ? h : 1;
}
PF_DEDUP_HD inline uint64_t nonzero(uint64_t w) { return w ? w : 1; }

// the two sums of one read's first L bases (plain restatement: a byte at a time)
PF_DEDUP_HD inline void read_sums(const char *seq, uint32_t L, bool second, uint64_t sum[2]) {
    for (uint32_t j = 0; 16ull * j < L; ++j) {
        uint64_t word = 0;
        for (uint32_t i = 0; i < WORD_BASES && 16 * j + i < L; ++i) word |= (uint64_t)code((uint8_t)seq[16 * j + i]) << (CODE_BITS * i);
        sum[0] += term(word, index_of(j, second), 0);
        sum[1] += term(word, index_of(j, second), 1);
    }
}
// the key of a unit: pair = false takes seq1 alone
PF_DEDUP_HD inline void key_of(const char *seq1, uint32_t n1, const char *seq2, uint32_t n2, bool pair, uint32_t bases, uint64_t key[2]) {
    const uint32_t l1 = covered(n1, bases), l2 = pair ? covered(n2, bases) : 0u;
    uint64_t sum[2] = {0, 0};
    read_sums(seq1, l1, false, sum);
    if (pair) read_sums(seq2, l2, true, sum);
    key[0] = close(sum[0], l1, l2, pair, 0);
    key[1] = close(sum[1], l1, l2, pair, 1);
}

PF_DEDUP_HD inline uint64_t home(uint64_t h1, uint64_t slots) { return h1 & (slots - 1); }
// the smallest power of two >= MIN_SLOTS, >= have, that holds entries + n at half load (0: beyond 2^62)
PF_DEDUP_HD inline uint64_t needed_slots(uint64_t have, uint64_t entries, uint64_t n) {
    uint64_t s = have < MIN_SLOTS ? MIN_SLOTS : have;
    if (entries + n > (1ull << 61)) return 0;
    while (s < 2 * (entries + n)) s <<= 1;
    return s;
}
PF_DEDUP_HD inline uint64_t round_slots(uint64_t want) {   // initial_slots as given -> the table's first size
    if (want == 0) return DEFAULT_SLOTS;
    uint64_t s = MIN_SLOTS;
    while (s < want && s < (1ull << 62)) s <<= 1;
    return s;
}
PF_DEDUP_HD inline uint32_t level_of(uint64_t copies) { return copies >= LEVELS ? LEVELS - 1 : (uint32_t)(copies - 1); }   // copies >= 1

}  // namespace pf_dedup
