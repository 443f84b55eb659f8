// csrc/host_pieces.h without a GPU: the owned buffers on stubs of the runtime's four allocation calls (plain malloc / free that
// count and can be told to fail, so that the address sanitizer sees a leak, a double free or a use after a free), and the piece
// cutter on tables in heap blocks of exactly their size.  Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
constexpr unsigned hipHostMallocDefault = 0;
static int g_allocs[2], g_frees[2], g_fail_in = -1;  // [0] device, [1] pinned; g_fail_in: the allocation that fails, counted down
static hipError_t stub_alloc(int kind, void **p, size_t bytes) {
    if (g_fail_in >= 0 && g_fail_in-- == 0) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    ++g_allocs[kind];
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc(0, p, bytes); }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return stub_alloc(1, p, bytes); }
static hipError_t hipFree(void *p) { return free(p), ++g_frees[0], hipSuccess; }
static hipError_t hipHostFree(void *p) { return free(p), ++g_frees[1], hipSuccess; }

#include "host_pieces.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #x); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

struct Slot {  // like the slots of bgzf.hip: no destructor of its own, so it moves with its buffers
    flx_dev_buf d;
    flx_pinned_buf h;
    bool busy = false;
};

static void buffers() {
    {
        flx_dev_buf b;
        CHECK(b.reserve(0) == hipSuccess && !b.p && g_allocs[0] == 0);  // nothing asked, nothing allocated
        CHECK(b.reserve(100) == hipSuccess && b.p && b.cap == 100 && g_allocs[0] == 1);
        void *first = b.p;
        b.as()[99] = 1;
        CHECK(b.reserve(50) == hipSuccess && b.reserve(100) == hipSuccess && b.p == first && b.cap == 100 && g_allocs[0] == 1);  // reused
        CHECK(b.reserve(101) == hipSuccess && b.cap == 101 && g_allocs[0] == 2 && g_frees[0] == 1);  // grown: the old block is gone
        b.as()[100] = 2;
        g_fail_in = 0;
        CHECK(b.reserve(500) == hipErrorOutOfMemory && !b.p && b.cap == 0 && g_frees[0] == 2);  // a failure leaves it empty ...
        CHECK(b.reserve(500) == hipSuccess && b.cap == 500 && g_allocs[0] == 3);                // ... and the next call tries again
        flx_dev_buf c(std::move(b));
        CHECK(!b.p && b.cap == 0 && c.cap == 500);
        flx_dev_buf d;
        CHECK(d.reserve(7) == hipSuccess);
        d = std::move(c);  // frees d's 7 bytes
        CHECK(!c.p && d.cap == 500 && g_frees[0] == 3);
        flx_dev_buf &self = d;
        d = std::move(self);
        CHECK(d.cap == 500 && d.p);
    }
    CHECK(g_allocs[0] == 4 && g_frees[0] == 4 && g_allocs[1] == 0);
    {
        std::vector<Slot> slots;
        slots.resize(2);
        CHECK(flx_reserve_all(slots[0].d, 10, slots[0].h, 20, slots[1].h, 30) == hipSuccess);
        void *keep = slots[0].h.p;
        slots.resize(9);  // the slots move, their buffers stay where they are
        CHECK(slots[0].h.p == keep && slots[0].h.cap == 20 && slots[1].h.cap == 30 && !slots[8].d.p);
        CHECK(g_allocs[0] == 5 && g_allocs[1] == 2 && g_frees[1] == 0);
        g_fail_in = 1;  // the second allocation fails: the third buffer is not asked
        CHECK(flx_reserve_all(slots[2].d, 1, slots[2].h, 2, slots[3].d, 3) == hipErrorOutOfMemory);
        CHECK(slots[2].d.cap == 1 && !slots[2].h.p && !slots[3].d.p && g_fail_in == -1);
        CHECK(flx_reserve_all(slots[2].d, 1, slots[2].h, 2, slots[3].d, 3) == hipSuccess && g_allocs[0] == 7 && g_allocs[1] == 3);  // only what is missing
    }
    CHECK(g_allocs[0] == g_frees[0] && g_allocs[1] == g_frees[1] && g_frees[0] == 7 && g_frees[1] == 3);
}

// rec_off of n records of the given sizes, in a heap block of exactly n + 1 words
static uint64_t *table(const std::vector<uint64_t> &sizes) {
    uint64_t *t = (uint64_t *)malloc((sizes.size() + 1) * 8);
    t[0] = 1000;  // (offsets need not begin at 0)
    for (size_t i = 0; i < sizes.size(); ++i) t[i + 1] = t[i] + sizes[i];
    return t;
}

static void cutter() {
    uint64_t *none = table({});
    CHECK(flx_piece_records(none, 0, 0, 100) == 0);  // no records: no piece, and rec_off[1] is not read
    free(none);
    uint64_t *one = table({500});
    CHECK(flx_piece_records(one, 0, 1, 100) == 1 && flx_piece_records(one, 1, 1, 100) == 0);  // a record larger than the piece is a piece
    free(one);
    uint64_t *t = table({40, 60, 1, 500, 100, 0, 0, 30});
    CHECK(flx_piece_records(t, 0, 8, 100) == 2);   // 40 + 60 fits exactly, + 1 does not
    CHECK(flx_piece_records(t, 0, 8, 99) == 1);
    CHECK(flx_piece_records(t, 2, 8, 100) == 1);   // the oversized record behind it is not taken along
    CHECK(flx_piece_records(t, 3, 8, 100) == 1);   // ... and goes alone
    CHECK(flx_piece_records(t, 4, 8, 100) == 3);   // empty records cost nothing; the last record would not fit
    CHECK(flx_piece_records(t, 4, 8, 130) == 4);   // up to the end of the table and not beyond
    CHECK(flx_piece_records(t, 4, 8, 130, 2) == 2 && flx_piece_records(t, 4, 8, 130, 1) == 1);  // the record cap
    const uint64_t c = flx_piece_records(t, 4, 8, 130);
    uint64_t *tab = (uint64_t *)malloc((c + 1) * 8);
    flx_piece_table(t, 4, c, tab);
    CHECK(tab[0] == 0 && tab[1] == 100 && tab[2] == 100 && tab[3] == 100 && tab[4] == 130);
    free(tab);
    free(t);
    uint64_t *many = table(std::vector<uint64_t>(kPieceRecords + 3, 0));  // the cap the callers use
    CHECK(flx_piece_records(many, 0, kPieceRecords + 3, 100) == kPieceRecords && flx_piece_records(many, kPieceRecords, kPieceRecords + 3, 100) == 3);
    free(many);
}

int main() {
    buffers();
    cutter();
    puts("ok");
    return 0;
}
