// qsplit.h — --split_window_q: reads split at low-quality windows in Phred mode.  The record core of qsplit.hip, shared by the
// kernels and the host walk, and like bam_record.h / bam_encode.h plain C++ that a HIP kernel and a host program both include.
// The reference has no counterpart: its --trim / --split need an external reference, and --min_window_q drops the whole read.
//
// Everything is defined on integers, so any parallel decomposition gives the answer of the serial walk below.
//   error table   E[b], uint32, for the byte b of a quality string: q = (signed char)b - 33; q <= 0 gives 2^32 - 1, otherwise
//                 min(2^32 - 1, floor(10^(-q/10) * 2^32 + 0.5)): the error probability of the base in units of 2^-32.  The 94 finite
//                 values (bytes 34..127) are literal constants below; tests/test_qsplit_host.py recomputes them with 60-digit decimals.
//   threshold     t = (uint64_t)floor((100 - Q) / 100 * 2^32) in IEEE double, Q = --split_window_q on the 0-100 scale of --min_window_q
//   windows       W = --window_size, L = the read's length, n = min(W, L) (a read of at most W bases is one window, itself, as in
//                 Read::get_window_quality).  The window that ends at base j, n - 1 <= j < L, is BAD iff the sum of E over the bases
//                 j - n + 1 .. j is greater than t * n (both in uint64: the sum stays below 2^63 for L < 2^31).
//   children      every base inside a bad window is removed; a child is a maximal run of the bases that are left, half-open and
//                 0-based like the children of flx_scores.  With the bad ends j_1 < j_2 < ...: the leading child [0, j_1 - n + 1) when
//                 that is not empty, between consecutive bad ends j < j' the child [j + 1, j' - W + 1) iff j' - j > W, and the
//                 trailing child [j_last + 1, L) when that is not empty.
//   first, last   the first kept base and one past the last kept base: 0 and L without a bad window, -1 and -1 when no base is kept
//                 (bad windows but no child: the read stays one entry and fails).  L = 0: no window, 0 and 0.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define QSPLIT_FN __host__ __device__ __forceinline__
#else
#define QSPLIT_FN inline
#endif

#define QSPLIT_E_MAX8 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u, 4294967295u
// E[0..255], eight entries a row; rows 4..15 hold the bytes 32..127 ('"' = 34 is quality 1, '~' = 126 is quality 93)
#define QSPLIT_ERROR_TABLE                                                                                        \
    QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8,                                                   \
    4294967295u, 4294967295u, 3411613790u, 2709941160u, 2152582778u, 1709857278u, 1358187913u, 1078847007u,       \
     856958639u,  680706443u,  540704347u,  429496730u,  341161379u,  270994116u,  215258278u,  170985728u,       \
     135818791u,  107884701u,   85695864u,   68070644u,   54070435u,   42949673u,   34116138u,   27099412u,       \
      21525828u,   17098573u,   13581879u,   10788470u,    8569586u,    6807064u,    5407043u,    4294967u,       \
       3411614u,    2709941u,    2152583u,    1709857u,    1358188u,    1078847u,     856959u,     680706u,       \
        540704u,     429497u,     341161u,     270994u,     215258u,     170986u,     135819u,     107885u,       \
         85696u,      68071u,      54070u,      42950u,      34116u,      27099u,      21526u,      17099u,       \
         13582u,      10788u,       8570u,       6807u,       5407u,       4295u,       3412u,       2710u,       \
          2153u,       1710u,       1358u,       1079u,        857u,        681u,        541u,        429u,       \
           341u,        271u,        215u,        171u,        136u,        108u,         86u,         68u,       \
            54u,         43u,         34u,         27u,         22u,         17u,         14u,         11u,       \
             9u,          7u,          5u,          4u,          3u,          3u,          2u,          2u,       \
    QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, \
    QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8, QSPLIT_E_MAX8

namespace qsplit {

// the host's copy of the table (the kernels keep theirs in constant memory and stage it in LDS: qsplit.hip)
static const uint32_t kErrorTable[256] = {QSPLIT_ERROR_TABLE};

// t of --split_window_q Q; false unless 0 < Q < 100
inline bool threshold(double q, uint64_t *t) {
    if (!(q > 0.0 && q < 100.0)) return false;
    volatile double frac = (100.0 - q) / 100.0;  // (rounded to double before the product, whatever the host's evaluation mode)
    volatile double scaled = frac * 4294967296.0;
    *t = (uint64_t)scaled;  // scaled is positive and below 2^32: the conversion is floor
    return true;
}

// The child rule for one bad end j behind the bad end `prev` (-1: j is the read's first): true when a child lies in front of
// j's window, [*start, *end).  Shared by the host walk and the detection kernel.
QSPLIT_FN bool child_before(int64_t prev, int64_t j, int64_t n, int64_t w, int32_t *start, int32_t *end) {
    if (prev < 0) {
        *start = 0;
        *end = (int32_t)(j - n + 1);
        return j - n + 1 > 0;
    }
    *start = (int32_t)(prev + 1);
    *end = (int32_t)(j - w + 1);
    return j - prev > w;
}

struct Children {
    std::vector<int32_t> ranges;  // (start, end) pairs
    int32_t first = 0, last = 0;
    bool any_bad = false;
};

// The serial walk over one quality string: the kernels' oracle.  Reads qual[0, L) and nothing else.
inline void qsplit_children_host(const uint8_t *qual, int64_t L, int64_t W, uint64_t t, Children *out) {
    out->ranges.clear();
    out->any_bad = false;
    out->first = 0;
    out->last = (int32_t)L;
    if (L <= 0 || W <= 0) return;
    const int64_t n = W < L ? W : L;
    const uint64_t limit = t * (uint64_t)n;
    uint64_t sum = 0;
    for (int64_t i = 0; i < n - 1; ++i) sum += kErrorTable[qual[i]];
    int64_t prev = -1;
    for (int64_t j = n - 1; j < L; ++j) {
        sum += kErrorTable[qual[j]];
        if (j >= n) sum -= kErrorTable[qual[j - n]];
        if (sum <= limit) continue;
        int32_t s, e;
        if (child_before(prev, j, n, W, &s, &e)) {
            out->ranges.push_back(s);
            out->ranges.push_back(e);
        }
        prev = j;
    }
    if (prev < 0) return;
    out->any_bad = true;
    if (prev + 1 < L) {
        out->ranges.push_back((int32_t)(prev + 1));
        out->ranges.push_back((int32_t)L);
    }
    out->first = out->ranges.empty() ? -1 : out->ranges.front();
    out->last = out->ranges.empty() ? -1 : out->ranges.back();
}

}  // namespace qsplit
