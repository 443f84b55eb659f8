// screen_hash.h — --exclude_k K: the contaminant screen with K-mers of 16 <= K <= 31 bases, kept as hashed 64-bit keys.  The host
// core of screen_hash.hip, and like screen.h plain C++ that a HIP kernel and a host program both include.
//
// The definition is screen.h's with 16 replaced by K, on integers:
//   the set X_K   every K-mer of either strand of the reference whose K bytes are all in ACGTacgt (the K-mers of the maximal ACGTacgt
//                 runs of at least K bases; no window spans two sequences)
//   forward code  A 0, C 1, G 2, T 3, the first base on top, in 2 K <= 62 bits
//   canonical key the smaller of the forward code and the code of the reverse complement.  A window is in X_K iff its canonical key
//                 is among the canonical keys of the reference, so the set stores canonical keys only: half the memory
//   hits          windows = max(0, L - K + 1); hits counts the i in [0, windows) whose K bytes are all in ACGTacgt and whose
//                 window is in X_K.  Threshold and decision are screen.h's.
// The table is open addressing over uint64_t slots: capacity a power of two, the slot of a key is mix(key) & (capacity - 1), probing
// is linear and wraps, an empty slot holds ~0 (no key of K <= 31 has bit 62 set).  Hits are sums of set memberships: the mixer, the
// capacity and the order of insertion cannot change a result.
#pragma once

#include "screen.h"

namespace screenk {

constexpr int kMinK = 16, kMaxK = 31;
constexpr uint64_t kEmpty = ~0ull;

SCREEN_FN uint32_t windows_of(int64_t length, int k) { return length >= k ? (uint32_t)(length - k + 1) : 0u; }

// the codes of all 2 K bits set: the largest forward code (all T)
SCREEN_FN uint64_t code_mask(int k) { return (1ull << (2 * k)) - 1ull; }

// the bases of a 64-bit word of 32 2-bit codes in reverse order
SCREEN_FN uint64_t reverse_codes(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    return (x >> 32) | (x << 32);
}

// the code of the reverse complement of a K-mer given by its forward code (the complement of a code c is 3 - c = ~c)
SCREEN_FN uint64_t revcomp_code(uint64_t fwd, int k) { return reverse_codes(~fwd) >> (64 - 2 * k); }

SCREEN_FN uint64_t canonical(uint64_t fwd, int k) {
    const uint64_t rc = revcomp_code(fwd, k);
    return fwd < rc ? fwd : rc;
}

// the forward code of the K bytes at s (all in ACGTacgt: the caller has looked)
SCREEN_FN uint64_t forward_code(const uint8_t *s, int k) {
    uint64_t c = 0;
    for (int i = 0; i < k; ++i) c = (c << 2) | (uint64_t)screen::code_of(s[i]);
    return c;
}

SCREEN_FN bool window_valid(const uint8_t *s, int k) {
    for (int i = 0; i < k; ++i)
        if (!screen::is_acgt(s[i])) return false;
    return true;
}

// the one mixer of the table (the finisher of MurmurHash3, a bijection of uint64)
SCREEN_FN uint64_t mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
SCREEN_FN uint64_t slot_of(uint64_t key, uint64_t capacity) { return mix(key) & (capacity - 1ull); }

// ---- the table on the host, exactly as the device builds and asks it (for one thread) ----
// the slot that holds `key`, or capacity if it is not stored.  A table without an empty slot is asked at most capacity times.
inline uint64_t find(const uint64_t *table, uint64_t capacity, uint64_t key) {
    uint64_t s = slot_of(key, capacity);
    for (uint64_t n = 0; n < capacity; ++n, s = (s + 1) & (capacity - 1)) {
        if (table[s] == key) return s;
        if (table[s] == kEmpty) return capacity;
    }
    return capacity;
}
// 1: the key took an empty slot, 0: it was stored already, -1: the table is full and does not hold it
inline int insert(uint64_t *table, uint64_t capacity, uint64_t key) {
    uint64_t s = slot_of(key, capacity);
    for (uint64_t n = 0; n < capacity; ++n, s = (s + 1) & (capacity - 1)) {
        if (table[s] == key) return 0;
        if (table[s] == kEmpty) {
            table[s] = key;
            return 1;
        }
    }
    return -1;
}

}  // namespace screenk
