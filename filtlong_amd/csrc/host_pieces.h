// host_pieces.h — what the host-to-host paths of bam.hip and bgzf.hip share: buffers that a slot owns, and the cut of a call into
// pieces of whole records.  Included behind the runtime's header; the four allocation calls are all it needs of it
// (tests/host_pieces_host.cpp runs it on stubs of them, under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

// A device (or pinned host) buffer owned by whoever holds it: it grows alone and only when it is too small (a free synchronises
// the device under every other stream), keeps what it has when asked for less, and frees itself.  Move-only, so that slots can
// live in a std::vector.  The owner synchronises the stream that uses the buffer before it lets go of it.
template <bool PINNED>
struct flx_owned_buf {
    void *p = nullptr;
    size_t cap = 0;

    flx_owned_buf() = default;
    flx_owned_buf(const flx_owned_buf &) = delete;
    flx_owned_buf &operator=(const flx_owned_buf &) = delete;
    flx_owned_buf(flx_owned_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    flx_owned_buf &operator=(flx_owned_buf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~flx_owned_buf() { release(); }

    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    template <class T = uint8_t>
    T *as() const { return (T *)p; }

  private:
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
};
using flx_dev_buf = flx_owned_buf<false>;
using flx_pinned_buf = flx_owned_buf<true>;

// reserve() of every (buffer, bytes) pair in turn, up to the first failure
inline hipError_t flx_reserve_all() { return hipSuccess; }
template <class B, class... Rest>
hipError_t flx_reserve_all(B &buf, size_t bytes, Rest &&...rest) {
    const hipError_t e = buf.reserve(bytes);
    return e != hipSuccess ? e : flx_reserve_all(rest...);
}

// A call is cut into pieces of whole records: records [k, k + c) of rec_off[0 .. n_rec], as many as stay within piece_bytes bytes
// and kPieceRecords records, and at least one (a record larger than the piece: the staging grows to it).  0 at k == n_rec.
constexpr uint64_t kPieceRecords = 1u << 20;
constexpr uint64_t kPieceMinTable = 4096;  // slots make room for at least this many records, so that small pieces find it made
inline uint64_t flx_piece_records(const uint64_t *rec_off, uint64_t k, uint64_t n_rec, uint64_t piece_bytes, uint64_t max_records = kPieceRecords) {
    if (k >= n_rec) return 0;
    uint64_t c = 1;
    while (k + c < n_rec && c < max_records && rec_off[k + c + 1] - rec_off[k] <= piece_bytes) ++c;
    return c;
}
// ... and the piece's own offset table, relative to its first byte: tab[0 .. c] (filled once the slot has room for c records)
inline void flx_piece_table(const uint64_t *rec_off, uint64_t k, uint64_t c, uint64_t *tab) {
    for (uint64_t j = 0; j <= c; ++j) tab[j] = rec_off[k + j] - rec_off[k];
}
