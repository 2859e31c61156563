// The two folded pieces of k_fast (manhattanslam_amd/csrc/msl_orb_fast.h) on the host, against the expressions they replace, which are kept
// here verbatim (namespace before): fast_score16 on (r, -r) pairs with the centre added once, and the quick test whose byte offset and widening
// are one byte permute per 16-bit pair (fast_quick4_at).  Built by tests/test_fast_fold_host.py, plain and with -fsanitize=address,undefined;
// exit status 0 = every case agrees.
#include "msl_orb_fast.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

using namespace msl::orb;

namespace before {   // the forms in use until this change, unchanged

s16x2 fast_pair(uint32_t w, int half) {
    const uint32_t h = half ? w >> 16 : w;
    return pk_from_bits((h & 0xFFu) | ((h & 0xFF00u) << 8));
}
uint32_t fast_bytes(uint32_t lo, uint32_t hi, int n) { return (lo >> (8 * n)) | (hi << (32 - 8 * n)); }
unsigned fast_quick4(uint32_t c, uint32_t r0, uint32_t r8, uint32_t r4, uint32_t r12, uint32_t r2, uint32_t r10, uint32_t r6, uint32_t r14, int th) {
    const s16x2 t = pk_make(th, th);
    uint32_t sign[2];
    for (int half = 0; half < 2; half++) {
        const s16x2 v = fast_pair(c, half);
        const s16x2 a0 = fast_pair(r0, half), a8 = fast_pair(r8, half), a4 = fast_pair(r4, half), a12 = fast_pair(r12, half);
        const s16x2 a2 = fast_pair(r2, half), a10 = fast_pair(r10, half), a6 = fast_pair(r6, half), a14 = fast_pair(r14, half);
        const s16x2 lo = pk_max(pk_max(pk_min(a0, a8), pk_min(a4, a12)), pk_max(pk_min(a2, a10), pk_min(a6, a14)));
        const s16x2 hi = pk_min(pk_min(pk_max(a0, a8), pk_max(a4, a12)), pk_min(pk_max(a2, a10), pk_max(a6, a14)));
        sign[half] = pk_bits(pk_sub(pk_add(lo, t), v)) | pk_bits(pk_sub(pk_add(v, t), hi));
    }
    return ((sign[0] >> 15) & 1u) | ((sign[0] >> 30) & 2u) | ((sign[1] >> 13) & 4u) | ((sign[1] >> 28) & 8u);
}
int fast_score16(int v, const int *ring) {
    s16x2 x[16], lo2[16], lo4[16];
    for (int k = 0; k < 16; k++) { const int d = v - ring[k]; x[k] = pk_make(d, -d); }
    for (int k = 0; k < 16; k++) lo2[k] = pk_min(x[k], x[(k + 1) & 15]);
    for (int k = 0; k < 16; k++) lo4[k] = pk_min(lo2[k], lo2[(k + 2) & 15]);
    s16x2 a = pk_make(-256, -256);
    for (int k = 0; k < 16; k++) a = pk_max(a, pk_min(pk_min(lo4[k], lo4[(k + 4) & 15]), x[(k + 8) & 15]));
    const int p = a.x, n = a.y;
    return (p > n ? p : n) - 1;
}

}  // namespace before

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

long checked = 0;
int failures = 0;

// ---- score: the ring against every centre value 0 .. 255 ----
void check_ring(const int *ring) {
    for (int v = 0; v < 256; v++) {
        const int want = before::fast_score16(v, ring), got = fast_score16(v, ring);
        checked++;
        if (want != got && failures++ < 5) {
            std::fprintf(stderr, "score: v %d: before %d, now %d, ring", v, want, got);
            for (int k = 0; k < 16; k++) std::fprintf(stderr, " %d", ring[k]);
            std::fprintf(stderr, "\n");
        }
    }
}

// ---- quick test ----
// the word the old form cut out n bytes into (lo, hi); n = 0 is lo itself (the kernel passed it as such: a shift by 32 is not defined)
uint32_t cut(uint32_t lo, uint32_t hi, int n) { return n ? before::fast_bytes(lo, hi, n) : lo; }

void check_pairs(uint32_t lo, uint32_t hi) {
    for (int n = 0; n < 4; n++)
        for (int half = 0; half < 2; half++) {
            const uint32_t want = pk_bits(before::fast_pair(cut(lo, hi, n), half)), got = pk_bits(fast_pair_at(FastSrc{lo, hi, n}, half));
            checked++;
            if (want != got && failures++ < 5) std::fprintf(stderr, "pair: lo %08x hi %08x n %d half %d: before %08x, now %08x\n", lo, hi, n, half, want, got);
        }
}

const int THS[4] = {0, 7, 20, 255};

// nine (lo, hi) strings; n[i] = the byte alignment of string i
void check_quick(const uint32_t w[9][2], const int n[9]) {
    for (int th : THS) {
        const unsigned want = before::fast_quick4(cut(w[0][0], w[0][1], n[0]), cut(w[1][0], w[1][1], n[1]), cut(w[2][0], w[2][1], n[2]), cut(w[3][0], w[3][1], n[3]),
                                                  cut(w[4][0], w[4][1], n[4]), cut(w[5][0], w[5][1], n[5]), cut(w[6][0], w[6][1], n[6]), cut(w[7][0], w[7][1], n[7]),
                                                  cut(w[8][0], w[8][1], n[8]), th);
        const unsigned got = fast_quick4_at(FastSrc{w[0][0], w[0][1], n[0]}, FastSrc{w[1][0], w[1][1], n[1]}, FastSrc{w[2][0], w[2][1], n[2]}, FastSrc{w[3][0], w[3][1], n[3]},
                                            FastSrc{w[4][0], w[4][1], n[4]}, FastSrc{w[5][0], w[5][1], n[5]}, FastSrc{w[6][0], w[6][1], n[6]}, FastSrc{w[7][0], w[7][1], n[7]},
                                            FastSrc{w[8][0], w[8][1], n[8]}, th);
        checked++;
        if (want != got && failures++ < 5) std::fprintf(stderr, "quick test: th %d: before %x, now %x\n", th, want, got);
    }
}
void check_quick_all_alignments(const uint32_t w[9][2]) {
    static const int KERNEL[9] = {3, 3, 3, 2, 0, 1, 1, 1, 1};   // centre, ring 0, 8, 4, 12, 2, 10, 6, 14 as k_fast passes them
    check_quick(w, KERNEL);
    for (int a = 0; a < 4; a++) { const int n[9] = {a, a, a, a, a, a, a, a, a}; check_quick(w, n); }
    int n[9];
    for (int i = 0; i < 9; i++) n[i] = (int)(rnd() & 3u);
    check_quick(w, n);
}

}  // namespace

int main(int argc, char **argv) {
    const long nRandom = argc > 1 ? std::atol(argv[1]) : 100000;
    int ring[16];
    // ---- score: structured rings ----
    for (int r : {0, 1, 127, 128, 254, 255}) { for (int k = 0; k < 16; k++) ring[k] = r; check_ring(ring); }   // all equal
    for (int base : {0, 1, 100, 128, 254, 255})
        for (int other : {0, 1, 99, 101, 128, 254, 255})   // one arc of exactly 8 and of exactly 9 brighter or darker than the rest, at every start
            for (int arc : {8, 9})
                for (int start = 0; start < 16; start++) {
                    for (int k = 0; k < 16; k++) ring[k] = base;
                    for (int j = 0; j < arc; j++) ring[(start + j) & 15] = other;
                    check_ring(ring);
                }
    for (unsigned m = 0; m < 65536u; m += 7u) { for (int k = 0; k < 16; k++) ring[k] = ((m >> k) & 1u) ? 255 : 0; check_ring(ring); }   // values 0 and 255 only
    // ---- score: random rings, full range and low contrast ----
    for (long i = 0; i < nRandom; i++) {
        if (i & 1) { for (int k = 0; k < 16; k++) ring[k] = (int)(rnd() & 255u); }
        else { const int base = (int)(rnd() % 226u); for (int k = 0; k < 16; k++) ring[k] = base + (int)(rnd() % 30u); }
        check_ring(ring);
    }
    // ---- quick test: pairs at every alignment, then the whole test ----
    for (uint32_t lo : {0u, 0xFFFFFFFFu, 0x03020100u, 0xFF00FF00u, 0x80FF7F01u})
        for (uint32_t hi : {0u, 0xFFFFFFFFu, 0x07060504u, 0x00FF00FFu, 0x017F80FEu}) check_pairs(lo, hi);
    for (int i = 0; i < 20000; i++) check_pairs(rnd() | (rnd() << 16), rnd() | (rnd() << 16));
    uint32_t w[9][2];
    for (uint32_t fill : {0u, 0xFFFFFFFFu, 0x5A5A5A5Au, 0x00FF00FFu, 0xFF00FF00u}) {   // flat, and 0 / 255 stripes
        for (int i = 0; i < 9; i++) w[i][0] = w[i][1] = fill;
        check_quick_all_alignments(w);
        for (int i = 1; i < 9; i++) { w[i][0] = ~fill; w[i][1] = ~fill; check_quick_all_alignments(w); }
    }
    for (int i = 0; i < 20000; i++) {
        const int kind = i % 3;
        const int base = (int)(rnd() % 256u), th = THS[(i / 3) & 3], span = 2 * (th > 120 ? 120 : th) + 5;
        for (int s = 0; s < 9; s++)
            for (int h = 0; h < 2; h++) {
                uint32_t x = 0;
                for (int b = 0; b < 4; b++) {
                    int v;
                    if (kind == 0) v = (int)(rnd() & 255u);                                            // full range
                    else if (kind == 1) v = base + (int)(rnd() % (unsigned)span) - span / 2;           // low contrast around a threshold
                    else v = base + ((int)(rnd() % 3u) - 1) * (th + (int)(rnd() % 2u));                // exact +-th and +-(th + 1) steps, ties
                    x |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * b);
                }
                w[s][h] = x;
            }
        check_quick_all_alignments(w);
    }
    std::printf("fast_fold_host: %ld comparisons, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
