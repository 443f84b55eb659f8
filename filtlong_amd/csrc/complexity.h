// complexity.h — --max_low_complexity: reads that are mostly simple repeats are dropped.  The host core of complexity.hip, and like
// screen.h and qsplit.h plain C++ that a HIP kernel and a host program both include.  The reference has no counterpart: its users run
// a second tool (fastp -y, prinseq -lc_method dust, the entropy filters of chopper and BBDuk) over the whole file in front of it.
//
// Everything is defined on integers, so any decomposition (spans, waves, lanes, chunks, ranks) gives the same answer.
//   window        64 consecutive bases, which hold 62 overlapping triplets.  A read of L bases has windows = max(0, L - 63) windows,
//                 one per start position.
//   counts        for a window whose 64 bytes are all in ACGTacgt (case folded, codes as screen::code_of), c_t is how often triplet
//                 kind t of the 64 kinds occurs among its 62 triplets.
//   score         S = sum over t of c_t (c_t - 1) / 2, the pairs of equal triplets, 0 .. 1891: the score of DUST and sdust at one
//                 fixed window length.
//   bad window    all 64 bytes are in ACGTacgt AND 10 S > T * 61, T an integer threshold on sdust's scale of tenths (10 .. 300,
//                 default 20: sdust's).  Equality is not bad: at T = 20, S = 122 is good and S = 123 is bad.  A window with any other
//                 byte is never bad (the rule the screen has for its windows).
//   decision      a read is low-complexity iff windows > 0 and (bad << 32) >= t * windows, t = screen::threshold(P): the screen's rule.
//                 Reads of fewer than 64 bases are never flagged.
//
// The sliding form (Slide below): for the triplet that comes in with count c, S += c, then ++c; for the one that goes out, --c, then
// S -= c.  The state of a window is a function of its 64 bytes alone, so a walk that starts with an empty state 63 bases in front of
// the end of the first window it owns gives that window — and every later one — the state the whole-read walk has there: the
// piece-wise walk below, which is what the kernel's lanes do.
#pragma once

#include <stdint.h>
#include <string.h>

#include "screen.h"

namespace complexity {

constexpr int kWindow = 64;              // bases of a window
constexpr int kTriplets = kWindow - 2;   // triplets of a window
constexpr int kWarmup = kWindow - 1;     // bases a fresh state has to see in front of the end of its first window
constexpr int kMinScore = 10, kMaxScore = 300, kDefaultScore = 20;
// The work item of k_complexity_bad: this many window start positions of one read, kLaneRun for every lane of a wave.  A lane walks
// kLaneRun + kWarmup bases for its kLaneRun windows.  The last span of a read has fewer windows: its lanes share them in shorter
// runs (lane_run), so a wave is done sooner instead of leaving most of its lanes idle.
constexpr int kLaneRun = 128;
constexpr int kSpan = 64 * kLaneRun;
static_assert(kSpan % kWindow == 0 && kLaneRun % 16 == 0, "a span is whole windows, a lane's run whole 16-byte loads");

// window starts per lane in a span of `windows` window starts (1 .. kSpan): a 64th of them, rounded up to whole 16-byte loads
SCREEN_FN uint32_t lane_run(uint32_t windows) {
    const uint32_t r = ((windows + 63u) / 64u + 15u) & ~15u;
    return r < (uint32_t)kLaneRun ? r : (uint32_t)kLaneRun;
}

SCREEN_FN uint32_t windows_of(int64_t length) { return length >= kWindow ? (uint32_t)(length - kWarmup) : 0u; }

SCREEN_FN bool score_valid(int64_t score_t) { return score_t >= kMinScore && score_t <= kMaxScore; }

// is a window of score S bad at threshold T (the window's bytes are all ACGTacgt)
SCREEN_FN bool bad(uint32_t S, uint32_t T) { return 10u * S > T * (uint32_t)(kWindow - 3); }

// S of the 64 bytes at w from scratch, or -1 if one of them is outside ACGTacgt
SCREEN_FN int32_t score_of_window(const uint8_t *w) {
    uint8_t c[64];
    for (int t = 0; t < 64; ++t) c[t] = 0;
    for (int i = 0; i < kWindow; ++i)
        if (!screen::is_acgt(w[i])) return -1;
    int32_t S = 0;
    for (int i = 0; i + 2 < kWindow; ++i) {
        const uint32_t t = (screen::code_of(w[i]) << 4) | (screen::code_of(w[i + 1]) << 2) | screen::code_of(w[i + 2]);
        S += c[t]++;
    }
    return S;
}

// The sliding state: the counts and S of the triplets that end inside the last 62 positions, the bytes outside ACGTacgt among the last
// 64, and the last two codes.  push(byte) takes the next base; afterwards full() says whether 64 bases are in and bad_now(T) whether
// the window that ends at that base is bad.  The three bytes of a triplet need not be valid: its kind is then any value, and the
// window is masked by `invalid`.
struct Slide {
    uint8_t count[64];
    uint8_t ring[kWindow];  // kinds of the last 62 triplets and validity of the last 64 bytes, by position mod 64
    uint8_t okring[kWindow];
    uint32_t S = 0, invalid = 0, seen = 0, last2 = 0;
    Slide() {
        memset(count, 0, sizeof count);
        memset(ring, 0, sizeof ring);
        memset(okring, 0, sizeof okring);
    }
    void push(uint8_t b) {
        const uint32_t slot = seen & (uint32_t)(kWindow - 1);
        if (seen >= (uint32_t)kWindow) {
            invalid -= okring[slot] ? 0u : 1u;  // the byte 64 back leaves ...
            const uint32_t out = ring[(seen - (uint32_t)kTriplets) & (uint32_t)(kWindow - 1)];  // ... and the triplet that began with it
            S -= --count[out];
        }
        const bool ok = screen::is_acgt(b);
        okring[slot] = ok ? 1 : 0;
        invalid += ok ? 0u : 1u;
        const uint32_t kind = ((last2 << 2) | screen::code_of(b)) & 63u;
        last2 = kind & 15u;
        if (seen >= 2u) {
            ring[slot] = (uint8_t)kind;
            S += count[kind]++;
        }
        ++seen;
    }
    bool full() const { return seen >= (uint32_t)kWindow; }
    bool bad_now(uint32_t T) const { return full() && invalid == 0 && bad(S, T); }
};

// bad windows of the read s[0 .. length): one walk over the whole read
inline uint32_t bad_windows(const uint8_t *s, int64_t length, uint32_t T) {
    Slide st;
    uint32_t n = 0;
    for (int64_t i = 0; i < length; ++i) {
        st.push(s[i]);
        n += st.bad_now(T) ? 1u : 0u;
    }
    return n;
}

// the same in pieces of `piece` window start positions: the windows that start in [p, p + piece) come from a fresh state that begins
// at base p, i.e. kWarmup bases in front of the end of the first of them, and walks to base p + piece + kWarmup - 1 at the most
inline uint32_t bad_windows_pieces(const uint8_t *s, int64_t length, uint32_t T, int64_t piece) {
    const int64_t windows = (int64_t)windows_of(length);
    uint32_t n = 0;
    for (int64_t p = 0; p < windows; p += piece) {
        const int64_t w1 = p + piece < windows ? p + piece : windows;
        Slide st;
        for (int64_t i = p; i < w1 + kWarmup; ++i) {
            st.push(s[i]);
            n += st.bad_now(T) ? 1u : 0u;
        }
    }
    return n;
}

// ... and exactly as the kernel cuts a read: spans of kSpan window starts, every span in 64 runs of lane_run(its windows)
inline uint32_t bad_windows_lanes(const uint8_t *s, int64_t length, uint32_t T) {
    const int64_t windows = (int64_t)windows_of(length);
    uint32_t n = 0;
    for (int64_t w0 = 0; w0 < windows; w0 += kSpan) {
        const int64_t w1 = w0 + kSpan < windows ? w0 + kSpan : windows;
        const int64_t run = (int64_t)lane_run((uint32_t)(w1 - w0));
        for (int64_t s0 = w0; s0 < w1; s0 += run) {
            const int64_t s1 = s0 + run < w1 ? s0 + run : w1;
            Slide st;
            for (int64_t i = s0; i < s1 + kWarmup; ++i) {
                st.push(s[i]);
                n += st.bad_now(T) ? 1u : 0u;
            }
        }
    }
    return n;
}

SCREEN_FN bool flagged(uint32_t bad_windows_, uint32_t windows, uint64_t t) { return screen::excluded(bad_windows_, windows, t); }

}  // namespace complexity
