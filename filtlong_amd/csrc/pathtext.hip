// pathtext.hip — a 16-mer set as a TEXT for the locus path of the cover kernels (kmerset.h: flx_locus; cover_wave.hip:
// k_kmer_cover_w<.., LOCUS>, cover_queue.hip: k_kmer_cover_q).  Three forms write the bases and the piece starts — the assembly itself
// (flx_build_assembly_text), and for a set with short reads in it (src/kmers.cpp:142-166) the two path forms below
// (flx_build_path_text) — and ONE finish (text_alloc / text_finish) gives each of them its padding, the U13 bits and the seed table,
// from nothing but the finished text.
//
// The locus path needs a text in which every 16-base window inside one piece is a member, and — for the refutation by unique
// 13-mers — in which every member IS such a window.  An assembly is that text for its own 16-mers.  For any other set the
// members are the edges of a de Bruijn graph over 15-mers (member x.C enters node C, member C.y leaves it; exact15 holds both
// nibbles per node), and a decomposition of the edges into PATHS gives the pieces: at every node the i-th entering member (in
// the order of its first base) is continued by the i-th leaving member (in the order of its last base), entering members
// without a partner end their path, leaving members without one start a path.  Where a node has more than one entering or
// leaving member the SEQUENCES the set was built from say which belong together: every 17-mer x.C.y of theirs whose two
// 16-mers are members is a witness for "x.C is continued by C.y" (kept in a small hash table of the branching nodes only), and
// witnessed pairs are matched first — then a path follows the genome through a repeated 15-mer and only ends where a whole
// 16-mer repeats (a wrong or missing witness costs speed, never exactness: any pairing gives a valid text).  Every member lies on exactly one path (or on
// a cycle: every member of a cycle becomes a path of its own), a path of m members is a piece of m + 15 bases, and along a
// genome the pairing is wrong only where a 15-mer repeats — about every 200 bases of a 5 Mbp genome, where the cover kernel
// seeds again inside the span.  Everything runs on the device: ranks from a popcount index of the bitmap, predecessor links,
// pointer jumping to (head, distance), lengths, offsets by an exclusive scan, the text.
//
// Round 4, second form (flx_build_path_text, first choice): the same construction one order higher.  At order 16 a piece ends
// wherever a 16-mer of the genome repeats (every ~580 bases of a read through a 5 Mbp genome even with the witnesses); the
// sequences the set was built from are longer than that.  So the graph is built over their 24-MERS (48 bits; a 23-mer of a 5 Mbp
// genome practically never repeats): every 24-mer of both strands whose nine 16-mers are all members, sorted and made unique
// (radix sort), linked by binary search, cut into paths exactly like the 16-mers above — a piece of m 24-mers is a text of m + 23
// bases in which every 16-base window is a member by construction.  Members that no such 24-mer holds (the ends of the
// sequences, 16-mers that only just made the count) become pieces of their own, so that every member is a window of the text
// (U13).
#include <cstring>
#include <vector>

#include "flx_internal.h"
#include "kmerset.h"
#include "rank_internal.h"

namespace {

// members per 256 bits of the bitmap (2^24 blocks)
__global__ void __launch_bounds__(256) k_pt_count256(const uint32_t *bm, int64_t *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 a = reinterpret_cast<const uint4 *>(bm)[2 * (size_t)i], b = reinterpret_cast<const uint4 *>(bm)[2 * (size_t)i + 1];
    cnt[i] = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
}

// index of member v among the members in increasing order
__device__ __forceinline__ uint32_t pt_rank(const uint32_t *bm, const int64_t *pre256, uint32_t v) {
    const uint32_t w = v >> 5;
    uint32_t r = (uint32_t)pre256[v >> 8];
    for (uint32_t k = w & ~7u; k < w; ++k) r += __popc(bm[k]);
    return r + __popc(bm[w] & ((1u << (v & 31)) - 1u));
}

__global__ void __launch_bounds__(256) k_pt_members(const uint32_t *bm, const int64_t *pre256, uint32_t *members) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t at = (uint32_t)pre256[i];
    for (uint32_t k = 0; k < 8; ++k) {
        uint32_t w = bm[8 * (size_t)i + k];
        while (w) {
            const int b = __ffs(w) - 1;
            w &= w - 1;
            members[at++] = ((8u * i + k) << 5) | (uint32_t)b;
        }
    }
}

// ---- witnesses at branching nodes: bit 4 x + y of a node's entry = "a sequence holds x.C.y" ----
struct PtWitness {
    uint32_t *keys;  // node + 1, 0 = empty
    uint32_t *vals;
    uint32_t mask;
};
__device__ __forceinline__ uint32_t pt_node_hash(uint32_t node, uint32_t mask) { return ((node * 0x9E3779B1u) >> 7) & mask; }
__device__ __forceinline__ bool pt_branching(uint32_t byte) { return (byte & 15u) && (byte >> 4) && (__popc(byte & 15u) > 1 || __popc(byte >> 4) > 1); }

__global__ void __launch_bounds__(256) k_pt_witness(const uint8_t *bases, const uint64_t *offsets, const uint64_t *pos_base, uint64_t n_seqs,
                                                    uint64_t n_pos, const uint8_t *exact15, PtWitness w) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_pos) return;
    const uint64_t lo = flx_seq_of(pos_base, n_seqs, g, 0);
    const uint64_t p = g - pos_base[lo];
    const uint64_t len = (lo + 1 < n_seqs ? pos_base[lo + 1] : n_pos) - pos_base[lo] + 15;
    if (p + 17 > len) return;
    const uint8_t *sq = bases + offsets[lo] + p;
    // the 17 codes of both strands (src/kmers.cpp:176-219): forward as they come, reverse from the other end in the reverse encoder's codes
    uint64_t f = 0, r = 0;
    for (int j = 0; j < 17; ++j) {
        f = (f << 2) | flx_base_fwd(sq[j]);
        r |= (uint64_t)flx_base_rev_code(sq[j]) << (2 * j);
    }
    const uint64_t two[2] = {f, r};
    for (int q = 0; q < 2; ++q) {
        const uint64_t v = two[q];  // 34 bits: x . C (30 bits) . y
        const uint32_t x = (uint32_t)(v >> 32) & 3u, node = (uint32_t)(v >> 2) & 0x3FFFFFFFu, y = (uint32_t)v & 3u;
        const uint32_t byte = exact15[node];
        if (!pt_branching(byte) || !((byte >> x) & 1u) || !((byte >> (4 + y)) & 1u)) continue;
        uint32_t h = pt_node_hash(node, w.mask);
        for (int probe = 0; probe < 64; ++probe) {
            const uint32_t old = atomicCAS(&w.keys[h], 0u, node + 1u);
            if (old == 0u || old == node + 1u) {
                atomicOr(&w.vals[h], 1u << (4 * x + y));
                break;
            }
            h = (h + 1) & w.mask;
        }
    }
}

// Which entering member (first base x) is continued by the leaving member with last base y at this node: witnessed pairs first
// (entering members in the order of x, each takes the smallest witnessed partner still free), then the rest in order.  4 = none.
__device__ __forceinline__ uint32_t pt_partner_of_out(uint32_t byte, uint32_t wit, uint32_t y) {
    const uint32_t in_mask = byte & 15u, out_mask = byte >> 4;
    uint32_t taken_out = 0, matched_in = 0, answer = 4;
    for (uint32_t x = 0; x < 4; ++x) {
        if (!((in_mask >> x) & 1u)) continue;
        const uint32_t c = out_mask & ((wit >> (4 * x)) & 15u) & ~taken_out;
        if (!c) continue;
        const uint32_t yy = (uint32_t)(__ffs(c) - 1);
        taken_out |= 1u << yy;
        matched_in |= 1u << x;
        if (yy == y) answer = x;
    }
    if ((taken_out >> y) & 1u) return answer;
    uint32_t free_in = in_mask & ~matched_in, free_out = out_mask & ~taken_out;
    const uint32_t rank = __popc(free_out & ((1u << y) - 1u));
    if (rank >= (uint32_t)__popc(free_in)) return 4;
    for (uint32_t k = 0; k < rank; ++k) free_in &= free_in - 1;
    return (uint32_t)(__ffs(free_in) - 1);
}

// predecessor on the path of every member (itself: the member starts a path)
__global__ void __launch_bounds__(256) k_pt_pred(const uint32_t *bm, const int64_t *pre256, const uint8_t *exact15, const uint32_t *members,
                                                 uint32_t n, PtWitness w, uint32_t *link, uint32_t *dist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = members[i];
    const uint32_t node = e >> 2, y = e & 3u;  // e leaves the node of its first 15 bases with its last base y
    const uint32_t byte = exact15[node];
    uint32_t wit = 0;
    if (pt_branching(byte)) {
        uint32_t h = pt_node_hash(node, w.mask);
        for (int probe = 0; probe < 64; ++probe) {
            const uint32_t k = w.keys[h];
            if (k == 0u) break;
            if (k == node + 1u) { wit = w.vals[h]; break; }
            h = (h + 1) & w.mask;
        }
    }
    const uint32_t x = pt_partner_of_out(byte, wit, y);
    uint32_t p = i;
    if (x < 4) {
        const uint32_t pe = (x << 30) | node;  // the entering member x.node
        if (pe != e) p = pt_rank(bm, pre256, pe);
    }
    link[i] = p;
    dist[i] = p == i ? 0u : 1u;
}

__global__ void __launch_bounds__(256) k_pt_jump(uint32_t n, const uint32_t *link_in, const uint32_t *dist_in, uint32_t *link_out, uint32_t *dist_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = link_in[i];
    dist_out[i] = dist_in[i] + dist_in[p];
    link_out[i] = link_in[p];
}

// after the jumps link[i] is the head of i's path — unless i lies on a cycle, where no member points at itself: such members become
// paths of their own.  Then the longest distance per head.
__global__ void __launch_bounds__(256) k_pt_heads(uint32_t n, uint32_t *link, uint32_t *dist, uint32_t *len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = link[i];
    if (link[h] != h) {  // (reads its neighbours' links of the jump phase: the rewrite goes to `len`'s kernel below, not here)
        dist[i] = 0x80000000u;  // marked; resolved in k_pt_lengths
    }
}
__global__ void __launch_bounds__(256) k_pt_lengths(uint32_t n, uint32_t *link, uint32_t *dist, uint32_t *len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dist[i] & 0x80000000u) {
        link[i] = i;
        dist[i] = 0;
    }
    atomicMax(&len[link[i]], dist[i] + 1u);
}
// bases of the piece every head starts: its elements and the `extra` bases in front of the first one's last
__global__ void __launch_bounds__(256) k_pt_piece_bases(uint32_t n, const uint32_t *link, const uint32_t *len, int extra, int64_t *bases) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bases[i] = link[i] == i ? (int64_t)len[i] + extra : 0;
}

__device__ __forceinline__ void pt_put(uint32_t *text_words, uint64_t t, uint32_t code, bool starts_piece) {
    uint32_t *w = text_words + 2 * ((t >> 4) + kLocusPad);
    if (code) atomicOr(w, code << (30 - 2 * (uint32_t)(t & 15)));
    if (starts_piece) atomicOr(w + 1, 1u << (uint32_t)(t & 15));
}

// every element (an edge of ORDER bases: a member at order 16, a 24-mer at order 24) writes its last base, the head of a piece
// the ORDER - 1 bases in front of it as well
template <typename Edge, int ORDER>
__global__ void __launch_bounds__(256) k_pt_text(uint32_t n, const Edge *edges, const uint32_t *link, const uint32_t *dist, const int64_t *off,
                                                 uint32_t *text_words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Edge e = edges[i];
    const uint64_t o = (uint64_t)off[link[i]];
    pt_put(text_words, o + (ORDER - 1) + dist[i], (uint32_t)(e & 3u), false);
    if (dist[i] == 0) {
        for (int j = 0; j < ORDER - 1; ++j) pt_put(text_words, o + j, (uint32_t)((e >> (2 * (ORDER - 1 - j))) & 3u), j == 0);
    }
}

__global__ void k_set_word_bits(uint32_t *word, uint32_t bits) { *word |= bits; }

// ---------------------------------------------------------------------------------------------------------------------
// order 24
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kNo24 = ~0ull;

// both strands' 24-mers at every start position of the sequences (key = 48 bits of codes, or kNo24 when one of its nine 16-mers is no member)
__global__ void __launch_bounds__(256) k24_emit(const uint8_t *bases, const uint64_t *offsets, const uint64_t *pos_base, uint64_t n_seqs, uint64_t n_pos,
                                                const uint32_t *present, uint64_t *keys) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_pos) return;
    const uint64_t lo = flx_seq_of(pos_base, n_seqs, g, 0);
    const uint64_t p = g - pos_base[lo];
    const uint64_t len = (lo + 1 < n_seqs ? pos_base[lo + 1] : n_pos) - pos_base[lo] + 15;
    uint64_t kf = kNo24, kr = kNo24;
    if (p + 24 <= len) {
        const uint8_t *sq = bases + offsets[lo] + p;
        uint64_t f = 0, r = 0;
        for (int j = 0; j < 24; ++j) {
            f = (f << 2) | flx_base_fwd(sq[j]);
            r |= (uint64_t)flx_base_rev_code(sq[j]) << (2 * j);
        }
        bool okf = true, okr = true;
        for (int w = 0; w < 9; ++w) {
            okf = okf && flx_test_bit(present, (uint32_t)(f >> (2 * w)));
            okr = okr && flx_test_bit(present, (uint32_t)(r >> (2 * w)));
        }
        if (okf) kf = f;
        if (okr) kr = r;
    }
    keys[2 * g] = kf;
    keys[2 * g + 1] = kr;
}

__global__ void __launch_bounds__(256) k24_flag(uint64_t n, const uint64_t *keys, uint32_t *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (keys[i] != kNo24 && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k24_compact(uint64_t n, const uint64_t *keys, const uint32_t *flag, const uint32_t *at, uint64_t *edges) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) edges[at[i]] = keys[i];
}

__device__ __forceinline__ uint32_t k24_lower_bound(const uint64_t *e, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (e[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// predecessor of every 24-mer on its path: entering and leaving edges of the node of its first 23 bases paired in order
__global__ void __launch_bounds__(256) k24_pred(const uint64_t *edges, uint32_t n, uint32_t *link, uint32_t *dist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = edges[i];
    const uint64_t node = e >> 2;  // 46 bits
    const uint32_t first_out = k24_lower_bound(edges, n, node << 2);
    const uint32_t out_rank = i - first_out;  // the leaving edges of a node are neighbours in the sorted array
    uint32_t in_idx[4], n_in = 0;
    for (uint64_t x = 0; x < 4; ++x) {
        const uint64_t key = (x << 46) | node;
        const uint32_t at = k24_lower_bound(edges, n, key);
        if (at < n && edges[at] == key) in_idx[n_in++] = at;
    }
    uint32_t p = i;
    if (out_rank < n_in && in_idx[out_rank] != i) p = in_idx[out_rank];
    link[i] = p;
    dist[i] = p == i ? 0u : 1u;
}

__global__ void __launch_bounds__(256) k24_cover(uint32_t n, const uint64_t *edges, uint32_t *covered) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = edges[i];
    for (int w = 0; w < 9; ++w) flx_set_bit(covered, (uint32_t)(e >> (2 * w)));
}
__global__ void __launch_bounds__(256) k24_leftover(const uint32_t *present, uint32_t *covered, uint64_t n_words) {  // covered := present & ~covered
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) covered[i] = present[i] & ~covered[i];
}

__global__ void __launch_bounds__(256) k24_text_leftover(uint32_t n, const uint32_t *members, uint64_t text_base, uint32_t *text_words) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = members[i];
    for (int j = 0; j < 16; ++j) pt_put(text_words, text_base + 16ull * i + j, (e >> (30 - 2 * j)) & 3u, j == 0);
}

// ---- the assembly form: one thread per base of the batch's sequences, which writes it into both strand copies ----
__global__ void __launch_bounds__(256) k_locus_text(const uint8_t *bases, const uint64_t *offsets, const uint64_t *pos_base,
                                                    uint64_t n_seqs, uint64_t n_pos, uint64_t text_base, uint32_t *text_words) {
    const uint64_t n_bases = n_pos + 15 * n_seqs;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_bases) return;
    const uint64_t lo = flx_seq_of(pos_base, n_seqs, g, 15);
    const uint64_t cum = pos_base[lo] + 15 * lo;  // bases of the sequences before it
    const uint64_t len = (lo + 1 < n_seqs ? pos_base[lo + 1] : n_pos) - pos_base[lo] + 15;
    const uint64_t o = g - cum;
    const uint8_t c = bases[offsets[lo] + o];
    const uint64_t tf = text_base + 2 * cum + o, tr = text_base + 2 * cum + len + (len - 1 - o);
    pt_put(text_words, tf, flx_base_fwd(c), o == 0);
    pt_put(text_words, tr, flx_base_rev_code(c), o == len - 1);
}

// ---- U13 and seeds from the text itself, for every form: one thread per text position ----
// U13 (kmerset.h), two passes over every 13-base window inside a piece: count its value (saturating at 2: two bitmaps of 4^13 bits),
// then mark the windows whose value was seen once
template <int PASS>
__global__ void __launch_bounds__(256) k_text_u13(uint32_t *text_words, uint64_t n_text, uint32_t *seen1, uint32_t *seen2) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_text || !flx_locus_in_piece((const uint2 *)text_words, n_text, t, 13)) return;
    const uint32_t v = flx_locus_kmer_at((const uint2 *)text_words, (uint32_t)t) >> 6;
    if (PASS == 0) {
        if (flx_set_bit(seen1, v)) flx_set_bit(seen2, v);
    } else if (!flx_test_bit(seen2, v)) {
        atomicOr(text_words + 2 * ((t >> 4) + kLocusPad) + 1, 0x10000u << (uint32_t)(t & 15));
    }
}
__global__ void __launch_bounds__(256) k_text_seed(const uint2 *text, uint64_t n_text, uint32_t *seed, uint32_t mask, int shift) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_text || !flx_locus_in_piece(text, n_text, t, 16)) return;
    const uint32_t k = flx_locus_kmer_at(text, (uint32_t)t);
    uint32_t h = flx_locus_hash(k, shift);
    for (;;) {
        const uint32_t old = atomicCAS(&seed[h], kLocusEmpty, (uint32_t)t);
        if (old == kLocusEmpty) break;
        if (flx_locus_kmer_at(text, old) == k) {  // the same 16-mer at another place of the text: the smallest position stays
            atomicMin(&seed[h], (uint32_t)t);
            break;
        }
        h = (h + 1) & mask;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the path section of both orders: predecessor links -> head and distance per element, piece lengths, piece offsets
// ---------------------------------------------------------------------------------------------------------------------
struct PathSection {
    flx_dbuf link0, link1, dist0, dist1, len, bases, off;
    uint32_t *link = nullptr, *dist = nullptr;  // after paths_from_links: the head of every element's path and its distance from it
    bool alloc(uint32_t n) {                    // (the pred kernel of the order writes link0 / dist0)
        for (flx_dbuf *b : {&link0, &link1, &dist0, &dist1, &len})
            if (hipMalloc(&b->p, (size_t)n * 4) != hipSuccess) return false;
        return hipMalloc(&bases.p, ((size_t)n + 1) * 8) == hipSuccess && hipMalloc(&off.p, ((size_t)n + 1) * 8) == hipSuccess;
    }
};

// Pointer jumping to (head, distance), the pieces' lengths in elements, and their offsets in the text by an exclusive scan of their
// bases (elements + `extra`: 15 at order 16, 23 at order 24); off[n] is the number of bases of all pieces.
int paths_from_links(flx_ctx *ctx, PathSection &ps, uint32_t n, int extra, void *ws, size_t ws_bytes) {
    hipStream_t st = ctx->stream;
    const uint32_t nb = (n + 255) / 256;
    uint32_t *link = ps.link0.as<uint32_t>(), *link2 = ps.link1.as<uint32_t>(), *dist = ps.dist0.as<uint32_t>(), *dist2 = ps.dist1.as<uint32_t>();
    int rounds = 1;
    while ((1ull << rounds) < (uint64_t)n + 1) ++rounds;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_pt_jump, dim3(nb), dim3(256), 0, st, n, link, dist, link2, dist2);
        std::swap(link, link2);
        std::swap(dist, dist2);
    }
    FLX_HIP(ctx, hipMemsetAsync(ps.len.p, 0, (size_t)n * 4, st));
    hipLaunchKernelGGL(k_pt_heads, dim3(nb), dim3(256), 0, st, n, link, dist, ps.len.as<uint32_t>());
    hipLaunchKernelGGL(k_pt_lengths, dim3(nb), dim3(256), 0, st, n, link, dist, ps.len.as<uint32_t>());
    FLX_HIP(ctx, hipMemsetAsync(ps.bases.p, 0, ((size_t)n + 1) * 8, st));
    hipLaunchKernelGGL(k_pt_piece_bases, dim3(nb), dim3(256), 0, st, n, link, ps.len.as<uint32_t>(), extra, ps.bases.as<int64_t>());
    FLX_CHECK(flx_exclusive_scan_i64(ctx, (uint64_t)n + 1, ps.bases.as<int64_t>(), ps.off.as<int64_t>(), ws, ws_bytes));
    ps.link = link;
    ps.dist = dist;
    return FLX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the finish of every form: room for the text, then — once the form has written its bases and piece starts — U13 and the seeds
// ---------------------------------------------------------------------------------------------------------------------
struct TextBuild {
    flx_dbuf text, seed, seen;  // seen: the two counting planes of U13 (4^13 bits each)
    uint64_t n_text = 0, n_words = 0, n_alloc = 0;
    int bits = 0;  // log2 of the seed table's slots
    uint32_t *words() { return text.as<uint32_t>(); }
};
constexpr size_t kU13Plane = (size_t)1 << (26 - 3);
constexpr uint64_t kBackPad = 68;

// Sizes and allocates the text of n_text positions, a seed table for n_keys keys (x 5/2, rounded up to a power of two, at least
// 2^10 slots) and the U13 planes BEFORE anything is built, and queues the padding, the seed fill and the plane clear.  No memory:
// FLX_OK with tb.text.p == nullptr, nothing left allocated and the HIP error cleared.
int text_alloc(flx_ctx *ctx, uint64_t n_text, uint64_t n_keys, TextBuild &tb) {
    hipStream_t st = ctx->stream;
    tb.n_text = n_text;
    tb.n_words = (n_text + 15) / 16;
    tb.n_alloc = tb.n_words + kLocusPad + kBackPad;
    tb.bits = 10;
    while ((1ull << tb.bits) < n_keys * 5 / 2) ++tb.bits;
    const uint64_t slots = 1ull << tb.bits;
    if (hipMalloc(&tb.text.p, tb.n_alloc * 8) != hipSuccess || hipMalloc(&tb.seed.p, slots * 4) != hipSuccess || hipMalloc(&tb.seen.p, 2 * kU13Plane) != hipSuccess) {
        for (flx_dbuf *b : {&tb.text, &tb.seed, &tb.seen}) {
            if (b->p) (void)hipFree(b->p);
            b->p = nullptr;
        }
        (void)hipGetLastError();
        return FLX_OK;
    }
    FLX_HIP(ctx, hipMemsetAsync(tb.text.p, 0, tb.n_alloc * 8, st));
    // padding: no window may start or end there
    std::vector<uint32_t> pad(2 * kBackPad);
    for (size_t i = 0; i < pad.size(); i += 2) { pad[i] = 0; pad[i + 1] = 0xffffu; }
    FLX_HIP(ctx, hipMemcpyAsync(tb.words(), pad.data(), 2 * kLocusPad * 4, hipMemcpyHostToDevice, st));
    FLX_HIP(ctx, hipMemcpyAsync(tb.words() + 2 * (kLocusPad + tb.n_words), pad.data(), pad.size() * 4, hipMemcpyHostToDevice, st));
    FLX_HIP(ctx, hipMemsetAsync(tb.seed.p, 0xff, slots * 4, st));
    FLX_HIP(ctx, hipMemsetAsync(tb.seen.p, 0, 2 * kU13Plane, st));
    return FLX_OK;
}

// The bases and piece starts are queued: the bits behind n_text, U13 in two passes and the seeds, all from the text itself.  Ends the
// form's timing bracket, waits, and hands text and seed table over to the caller (`loc` describes them).
int text_finish(flx_ctx *ctx, TextBuild &tb, flx_time_scope &timed, uint32_t **text_out, uint32_t **seed_out, flx_locus *loc) {
    hipStream_t st = ctx->stream;
    uint32_t *text = tb.words(), *seed = tb.seed.as<uint32_t>();
    // the last word's bases behind the text must not look like the start of anything: a piece "starts" at n_text
    if (tb.n_text % 16)
        hipLaunchKernelGGL(k_set_word_bits, dim3(1), dim3(1), 0, st, text + 2 * (kLocusPad + tb.n_words - 1) + 1, 0xffffu & ~((1u << (tb.n_text % 16)) - 1u));
    uint32_t *seen1 = tb.seen.as<uint32_t>(), *seen2 = seen1 + kU13Plane / 4;
    const unsigned blocks = (unsigned)((tb.n_text + 255) / 256);
    const uint32_t mask = (uint32_t)((1ull << tb.bits) - 1);
    hipLaunchKernelGGL(k_text_u13<0>, dim3(blocks), dim3(256), 0, st, text, tb.n_text, seen1, seen2);
    hipLaunchKernelGGL(k_text_u13<1>, dim3(blocks), dim3(256), 0, st, text, tb.n_text, seen1, seen2);
    hipLaunchKernelGGL(k_text_seed, dim3(blocks), dim3(256), 0, st, (const uint2 *)text, tb.n_text, seed, mask, 32 - tb.bits);
    timed.end();
    FLX_HIP(ctx, hipGetLastError());
    FLX_HIP(ctx, hipStreamSynchronize(st));
    loc->text = (const uint2 *)text;
    loc->n_alloc = (uint32_t)tb.n_alloc;
    loc->n_text = tb.n_text;
    loc->seed = seed;
    loc->seed_mask = mask;
    loc->seed_shift = 32 - tb.bits;
    *text_out = text;
    *seed_out = seed;
    tb.text.p = tb.seed.p = nullptr;
    return FLX_OK;
}

}  // namespace

// The assembly form (kmerset.h): for every sequence its forward strand, then its reverse strand.
int flx_build_assembly_text(flx_ctx *ctx, const flx_seq_batch *batches, size_t n_batches, uint32_t **text_out, uint32_t **seed_out, flx_locus *loc) {
    *text_out = nullptr;
    *seed_out = nullptr;
    uint64_t n_text = 0, n_windows = 0;
    for (size_t b = 0; b < n_batches; ++b) {
        n_text += 2 * (batches[b].n_pos + 15 * batches[b].n_seqs);
        n_windows += 2 * batches[b].n_pos;
    }
    if (n_windows == 0 || n_text > (1ull << 28)) return FLX_OK;
    TextBuild tb;
    FLX_CHECK(text_alloc(ctx, n_text, n_windows, tb));
    if (!tb.text.p) return FLX_OK;
    flx_time_scope timed(ctx, "flx_kmerset_locus_build");
    uint64_t text_base = 0;
    for (size_t b = 0; b < n_batches; ++b) {
        const uint64_t n_bases = batches[b].n_pos + 15 * batches[b].n_seqs;
        if (n_bases)
            hipLaunchKernelGGL(k_locus_text, dim3((unsigned)((n_bases + 255) / 256)), dim3(256), 0, ctx->stream, batches[b].bases, batches[b].offsets,
                               batches[b].pos_base, batches[b].n_seqs, batches[b].n_pos, text_base, tb.words());
        text_base += 2 * n_bases;
    }
    return text_finish(ctx, tb, timed, text_out, seed_out, loc);
}

// Order 24 (see the file header).  *text_out stays nullptr when this form cannot be built (no sequences, too many, no memory):
// the caller then takes the order-16 form below.
static int build_path_text_k24(flx_ctx *ctx, const uint32_t *present, uint64_t n_members, const flx_seq_batch *batches, size_t n_batches,
                               uint32_t **text_out, uint32_t **seed_out, flx_locus *loc) {
    hipStream_t st = ctx->stream;
    uint64_t n_pos = 0;
    for (size_t b = 0; b < n_batches; ++b) n_pos += batches[b].n_pos;
    if (n_pos == 0 || 2 * n_pos >= (1ull << 32)) return FLX_OK;
    const uint64_t nk = 2 * n_pos;
    auto alloc = [&](flx_dbuf &b, size_t bytes) { return hipMalloc(&b.p, bytes) == hipSuccess; };
    flx_dbuf k0, k1, v0, v1, ws, flag, at;
    const size_t ws_bytes = flx_radix_sort_workspace(nk + 1);
    if (!alloc(k0, nk * 8) || !alloc(k1, nk * 8) || !alloc(v0, nk * 4) || !alloc(v1, nk * 4) || !alloc(ws, ws_bytes) || !alloc(flag, (nk + 1) * 4) ||
        !alloc(at, (nk + 1) * 4)) {
        (void)hipGetLastError();
        return FLX_OK;
    }
    flx_time_scope timed(ctx, "flx_kmerset_locus_build");
    uint64_t done = 0;
    for (size_t b = 0; b < n_batches; ++b) {
        if (!batches[b].n_pos) continue;
        hipLaunchKernelGGL(k24_emit, dim3((unsigned)((batches[b].n_pos + 255) / 256)), dim3(256), 0, st, batches[b].bases, batches[b].offsets, batches[b].pos_base,
                           batches[b].n_seqs, batches[b].n_pos, present, k0.as<uint64_t>() + 2 * done);
        done += batches[b].n_pos;
    }
    uint64_t *sk = nullptr;
    uint32_t *sv = nullptr;
    FLX_CHECK(flx_radix_sort_pairs(ctx, nk, k0.as<uint64_t>(), k1.as<uint64_t>(), v0.as<uint32_t>(), v1.as<uint32_t>(), ws.p, ws_bytes, &sk, &sv));
    FLX_HIP(ctx, hipMemsetAsync(flag.p, 0, (nk + 1) * 4, st));
    hipLaunchKernelGGL(k24_flag, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, nk, sk, flag.as<uint32_t>());
    FLX_CHECK(flx_exclusive_scan_u32(ctx, nk + 1, flag.as<uint32_t>(), at.as<uint32_t>(), ws.p, ws_bytes));
    uint32_t m = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&m, at.as<uint32_t>() + nk, 4, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    if (m == 0 || m > (1u << 27)) return FLX_OK;
    uint64_t *edges = sk == k0.as<uint64_t>() ? k1.as<uint64_t>() : k0.as<uint64_t>();  // the buffer the sort did not end in
    hipLaunchKernelGGL(k24_compact, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, nk, sk, flag.as<uint32_t>(), at.as<uint32_t>(), edges);
    const uint32_t nb = (m + 255) / 256;
    PathSection ps;
    flx_dbuf d_cov, d_cnt, d_pre, d_left, ws2;
    const uint64_t n_blocks = 1ull << 24;
    const size_t ws2_bytes = std::max(flx_radix_sort_workspace(n_blocks + 1), flx_radix_sort_workspace((uint64_t)m + 1));
    if (!ps.alloc(m) || !alloc(d_cov, (size_t)1 << 29) || !alloc(d_cnt, (n_blocks + 1) * 8) || !alloc(d_pre, (n_blocks + 1) * 8) || !alloc(ws2, ws2_bytes)) {
        (void)hipGetLastError();
        return FLX_OK;
    }
    hipLaunchKernelGGL(k24_pred, dim3(nb), dim3(256), 0, st, edges, m, ps.link0.as<uint32_t>(), ps.dist0.as<uint32_t>());
    FLX_CHECK(paths_from_links(ctx, ps, m, 23, ws2.p, ws2_bytes));
    // members no 24-mer holds
    FLX_HIP(ctx, hipMemsetAsync(d_cov.p, 0, (size_t)1 << 29, st));
    hipLaunchKernelGGL(k24_cover, dim3(nb), dim3(256), 0, st, m, edges, d_cov.as<uint32_t>());
    hipLaunchKernelGGL(k24_leftover, dim3(8192), dim3(256), 0, st, present, d_cov.as<uint32_t>(), (uint64_t)1 << 27);
    FLX_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, (n_blocks + 1) * 8, st));
    hipLaunchKernelGGL(k_pt_count256, dim3((unsigned)(n_blocks / 256)), dim3(256), 0, st, d_cov.as<uint32_t>(), d_cnt.as<int64_t>());
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_blocks + 1, d_cnt.as<int64_t>(), d_pre.as<int64_t>(), ws2.p, ws2_bytes));
    int64_t path_bases = 0, n_left = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&path_bases, ps.off.as<int64_t>() + m, 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipMemcpyAsync(&n_left, d_pre.as<int64_t>() + n_blocks, 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t n_text = (uint64_t)path_bases + 16ull * (uint64_t)n_left;
    if (n_text == 0 || n_text > (1ull << 28) || (uint64_t)n_left > n_members) return FLX_OK;
    if (n_left > 0 && !alloc(d_left, (size_t)n_left * 4)) {
        (void)hipGetLastError();
        return FLX_OK;
    }
    TextBuild tb;
    FLX_CHECK(text_alloc(ctx, n_text, n_members, tb));
    if (!tb.text.p) return FLX_OK;
    hipLaunchKernelGGL((k_pt_text<uint64_t, 24>), dim3(nb), dim3(256), 0, st, m, edges, ps.link, ps.dist, ps.off.as<int64_t>(), tb.words());
    if (n_left > 0) {
        hipLaunchKernelGGL(k_pt_members, dim3((unsigned)(n_blocks / 256)), dim3(256), 0, st, d_cov.as<uint32_t>(), d_pre.as<int64_t>(), d_left.as<uint32_t>());
        hipLaunchKernelGGL(k24_text_leftover, dim3((unsigned)((n_left + 255) / 256)), dim3(256), 0, st, (uint32_t)n_left, d_left.as<uint32_t>(), (uint64_t)path_bases, tb.words());
    }
    return text_finish(ctx, tb, timed, text_out, seed_out, loc);
}

// The path forms (kmerset.h) for the members of `present` (n_members of them; exact15 is their pair table): order 24 first, then —
// here — order 16.
int flx_build_path_text(flx_ctx *ctx, const uint32_t *present, const uint8_t *exact15, uint64_t n_members, const flx_seq_batch *batches,
                        size_t n_batches, uint32_t **text_out, uint32_t **seed_out, flx_locus *loc) {
    *text_out = nullptr;
    *seed_out = nullptr;
    if (n_members == 0 || n_members > (1ull << 27)) return FLX_OK;
    {
        const char *order = getenv("FLX_KMER_TEXT_ORDER");  // "16": the order-16 form only (second implementation; tests, A/B)
        if (!(order && strcmp(order, "16") == 0)) {
            FLX_CHECK(build_path_text_k24(ctx, present, n_members, batches, n_batches, text_out, seed_out, loc));
            if (*text_out) return FLX_OK;
        }
    }
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)n_members;
    const uint32_t nb = (n + 255) / 256;
    const uint64_t n_blocks = 1ull << 24;
    PathSection ps;
    flx_dbuf d_cnt, d_pre, d_members, d_ws, d_wkeys, d_wvals;
    const uint32_t wit_slots = 1u << 22;  // (a 5 Mbp genome has ~1e5 branching 15-mers; what does not fit is paired by order)
    const size_t ws_bytes = std::max(flx_radix_sort_workspace(n_blocks + 1), flx_radix_sort_workspace((uint64_t)n + 1));
    auto alloc = [&](flx_dbuf &b, size_t bytes) { return hipMalloc(&b.p, bytes) == hipSuccess; };
    if (!alloc(d_cnt, (n_blocks + 1) * 8) || !alloc(d_pre, (n_blocks + 1) * 8) || !alloc(d_members, (size_t)n * 4) || !ps.alloc(n) || !alloc(d_ws, ws_bytes) ||
        !alloc(d_wkeys, (size_t)wit_slots * 4) || !alloc(d_wvals, (size_t)wit_slots * 4)) {
        (void)hipGetLastError();
        return FLX_OK;
    }
    flx_time_scope timed(ctx, "flx_kmerset_locus_build");
    FLX_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, (n_blocks + 1) * 8, st));
    hipLaunchKernelGGL(k_pt_count256, dim3((unsigned)(n_blocks / 256)), dim3(256), 0, st, present, d_cnt.as<int64_t>());
    FLX_CHECK(flx_exclusive_scan_i64(ctx, n_blocks + 1, d_cnt.as<int64_t>(), d_pre.as<int64_t>(), d_ws.p, ws_bytes));
    hipLaunchKernelGGL(k_pt_members, dim3((unsigned)(n_blocks / 256)), dim3(256), 0, st, present, d_pre.as<int64_t>(), d_members.as<uint32_t>());
    PtWitness wit;
    wit.keys = d_wkeys.as<uint32_t>();
    wit.vals = d_wvals.as<uint32_t>();
    wit.mask = wit_slots - 1;
    FLX_HIP(ctx, hipMemsetAsync(wit.keys, 0, (size_t)wit_slots * 4, st));
    FLX_HIP(ctx, hipMemsetAsync(wit.vals, 0, (size_t)wit_slots * 4, st));
    for (size_t b = 0; b < n_batches; ++b)
        if (batches[b].n_pos)
            hipLaunchKernelGGL(k_pt_witness, dim3((unsigned)((batches[b].n_pos + 255) / 256)), dim3(256), 0, st, batches[b].bases, batches[b].offsets,
                               batches[b].pos_base, batches[b].n_seqs, batches[b].n_pos, exact15, wit);
    hipLaunchKernelGGL(k_pt_pred, dim3(nb), dim3(256), 0, st, present, d_pre.as<int64_t>(), exact15, d_members.as<uint32_t>(), n, wit, ps.link0.as<uint32_t>(),
                       ps.dist0.as<uint32_t>());
    FLX_CHECK(paths_from_links(ctx, ps, n, 15, d_ws.p, ws_bytes));
    int64_t n_text = 0;
    FLX_HIP(ctx, hipMemcpyAsync(&n_text, ps.off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    FLX_HIP(ctx, hipStreamSynchronize(st));
    if (n_text <= 0 || (uint64_t)n_text > (1ull << 28)) return FLX_OK;
    TextBuild tb;
    FLX_CHECK(text_alloc(ctx, (uint64_t)n_text, n, tb));
    if (!tb.text.p) return FLX_OK;
    hipLaunchKernelGGL((k_pt_text<uint32_t, 16>), dim3(nb), dim3(256), 0, st, n, d_members.as<uint32_t>(), ps.link, ps.dist, ps.off.as<int64_t>(), tb.words());
    return text_finish(ctx, tb, timed, text_out, seed_out, loc);
}
