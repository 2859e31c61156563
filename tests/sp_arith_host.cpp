// The float / double identities of the superpixel kernels (manhattanslam_amd/csrc/msl_sf_sp_arith.h) on the host, bit for bit against the literal
// expressions of the reference written here.
//   div100     sp_div100_of_float(p) against (double)p / 100.0: every float with a zero low mantissa byte, the 64 neighbours of every power of two,
//              the denormal boundaries (--all: every one of the 2 139 095 040 finite non-negative floats); q0 = p * 0.01 alone must be wrong somewhere
//   cost       sp_cost_add_intensity / sp_cost_add_depth against calculateCost's two double additions, on random and edge pairs
//   newton     sp_newton_delta against (float)((double)(-sumA) / ((double)sumB + 10.0)) for all 257 denominators x edge numerators (zeros, denormals,
//              FLT_MAX, infinities, NaNs) and a strided sweep of all bit patterns; the comparisons with 0.01 and 0.2 around the constants and on the sweep
//   groups     the transposed 16-lane sums (sp_group_sum4 / sp_group_sum10 + sp_hessian_store) on arrays of 16 doubles against the one-value butterfly, on
//              inputs whose sums depend on the order (tests/sp_arith_inputs.py generates the same ones for the GPU test; `checksum` pins that)
// Built with -fsanitize=address,undefined -ffp-contract=off by tests/test_sp_arith_host.py; exit status 0 = every case agrees.
#include "msl_sf_sp_arith.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

using namespace msl::sf;

namespace {

long long checked = 0;
int failures = 0;

float f_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
uint32_t b_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
uint64_t b_of(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
double d_of(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
// (the literal expressions below go through volatile values: evaluated at run time, operation by operation)
uint64_t splitmix(uint64_t i) {
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void fail(const char *what, double a, double b, double got, double want) {
    if (failures++ < 10) std::fprintf(stderr, "%s(%a, %a): %a, literal %a\n", what, a, b, got, want);
}

// ---- item 1 ----
long long q0_wrong = 0;
void check_div100(uint32_t bits) {
    const float p = f_of(bits);
    volatile double x = (double)p;
    const double want = x / 100.0, got = sp_div100_of_float(p), two = sp_div100_of_double((double)p);
    checked++;
    if (b_of(got) != b_of(want)) fail("div100_of_float", p, 0, got, want);
    if (b_of(two) != b_of(want)) fail("div100_of_double", p, 0, two, want);
    if (b_of(x * 0.01) != b_of(want)) q0_wrong++;
}
void div100_quick() {
    for (uint32_t b = 0; b < 0x7F800000u; b += 256) check_div100(b);                       // zero low mantissa byte
    for (uint32_t e = 1; e < 255; e++)                                                      // 32 below, 32 from each power of two (e = 1: the denormal boundary)
        for (uint32_t b = (e << 23) - 32; b < (e << 23) + 32; b++) check_div100(b);
    for (uint32_t b = 0; b < 64; b++) check_div100(b);                                      // zero and the smallest denormals
    for (uint32_t b = 0x7F800000u - 64; b < 0x7F800000u; b++) check_div100(b);              // up to FLT_MAX
    for (int v = 0; v <= 255; v++) check_div100(b_of((float)v * (float)v));                 // the squares of whole intensity differences
}
void div100_all() {
    for (uint32_t b = 0; b < 0x7F800000u; b++) check_div100(b);
}

// ---- item 2 ----
void check_cost(float n, float d) {
    volatile float nv = n, dv = d;
    float wantI, wantD;
    {
        float nodepthCost = nv;
        const float intensityDiff = dv;
        nodepthCost = (float)((double)nodepthCost + (double)(intensityDiff * intensityDiff) / 100.0);
        wantI = nodepthCost;
    }
    {
        const float nodepthCost = nv, inverseDepthDiff = dv;
        volatile double prod = (double)(inverseDepthDiff * inverseDepthDiff) * 400.0;   // (volatile: rounded before the addition whatever the compiler's contraction rule)
        wantD = (float)((double)nodepthCost + prod);
    }
    const float gotI = sp_cost_add_intensity(n, d), gotD = sp_cost_add_depth(n, d);
    checked += 2;
    // (the division's contract is a FINITE dividend -- intensities are <= 255; an infinite square gives NaN in the one-step and in the two-step form alike)
    if (std::isfinite(dv * dv) && b_of(gotI) != b_of(wantI) && !(std::isnan(gotI) && std::isnan(wantI))) fail("cost_add_intensity", n, d, gotI, wantI);
    if (b_of(gotD) != b_of(wantD) && !(std::isnan(gotD) && std::isnan(wantD))) fail("cost_add_depth", n, d, gotD, wantD);
}
void cost_cases(long long nrandom) {
    const float edge[] = {0.0f, -0.0f, f_of(1), f_of(0x007FFFFFu), FLT_MIN, 1.0f, 0.1f, 0.05f, 255.0f, 3.0f, 1e-3f, 1e3f, 1.8446744e19f /* 2^64: its square overflows */,
                          1e19f, FLT_MAX, f_of(0x3F7FFFFFu), f_of(0x3F800001u), 16777215.0f, 65535.0f, 1e-20f, 1e-23f};
    for (float n : edge)
        for (float d : edge) { check_cost(n, d); check_cost(n, -d); }
    for (long long i = 0; i < nrandom; i++) {
        const uint64_t z = splitmix(0x100000000ull + (uint64_t)i);
        float n, d;
        switch (i & 3) {
        case 0: n = f_of((uint32_t)z & 0x7FFFFFFFu); d = f_of((uint32_t)(z >> 32)); break;                                   // any two bit patterns
        case 1: n = (float)((z & 0xFFFFF) * (1.0 / 4096.0)); d = (float)(((z >> 20) & 0xFFFFF) * (1.0 / 1048576.0)); break;   // costs up to 256, inverse depths up to 1
        case 2: n = (float)(z & 0xFFFF) * 0.0625f; d = f_of(0x30000000u + (uint32_t)((z >> 32) & 0x0FFFFFFFu)); break;       // quarter-squares against any magnitude
        default: n = f_of(0x3A000000u + (uint32_t)(z & 0x0BFFFFFFu)); d = f_of(0x3A000000u + (uint32_t)((z >> 32) & 0x07FFFFFFu)); break;
        }
        if (std::isnan(n) || std::isnan(d)) continue;
        check_cost(n, d);
    }
}

// ---- item 3 ----
void check_newton(float sumA, int inr) {
    volatile float av = sumA;
    const float sumB = (float)(2 * inr);
    volatile double den = (double)sumB + 10.0;
    const float want = (float)((double)(-av) / den);
    const float got = sp_newton_delta(sumA, inr), lit = sp_newton_delta_literal(sumA, inr);
    checked++;
    if (b_of(got) != b_of(want)) fail("newton_delta", sumA, inr, got, want);
    if (b_of(lit) != b_of(want)) fail("newton_delta_literal", sumA, inr, lit, want);
}
void check_cmp(float x) {
    volatile float xv = x;
    checked++;
    if (sp_lt_001(x) != ((double)xv < 0.01) || sp_gt_001(x) != ((double)xv > 0.01) || sp_gt_neg001(x) != ((double)xv > -0.01) || sp_lt_02(x) != ((double)xv < 0.2))
        fail("comparison with 0.01 / 0.2", x, 0, 0, 0);
}
void newton_cases(uint32_t stride) {
    const uint32_t edge[] = {0x00000000u, 0x00000001u, 0x00000002u, 0x007FFFFFu, 0x00800000u, 0x00800001u, 0x3F800000u, 0x3F7FFFFFu, 0x3F800001u, 0x40490FDBu,
                             0x7F7FFFFFu, 0x7F7FFFFEu, 0x7F800000u, 0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 0x7FA55555u, 0x3C23D70Au, 0x3C23D70Bu, 0x3C23D709u,
                             0x41200000u, 0x43828000u, 0x4B7FFFFFu, 0x0A000001u, 0x75555555u};
    for (int inr = 0; inr <= SP_NEWTON_MAX_INR; inr++)
        for (uint32_t e : edge) { check_newton(f_of(e), inr); check_newton(f_of(e | 0x80000000u), inr); }
    int inr = 0;
    for (uint64_t b = 0; b < 0x100000000ull; b += stride) {
        check_newton(f_of((uint32_t)b), inr);
        check_cmp(f_of((uint32_t)b));
        inr = inr == SP_NEWTON_MAX_INR ? 0 : inr + 1;
    }
    for (uint32_t c : {b_of(0.01f), b_of(0.2f), 0u, 0x7F800000u, 0x7FC00000u, 0x00800000u})
        for (int k = -64; k <= 64; k++) {
            const uint32_t b = c + (uint32_t)k;
            check_cmp(f_of(b)); check_cmp(f_of(b ^ 0x80000000u));
        }
}

// ---- item 4: the lane operations on arrays of 16 doubles ----
struct Lanes { double v[16]; };
struct ArrayOps {
    static int source(int ctrl, int i) {   // the lane whose value a DPP move with this control hands to lane i of the row
        if (ctrl >= 0x121 && ctrl <= 0x12F) return (i - (ctrl - 0x120)) & 15;                  // row_ror:n
        return (i & ~3) | ((ctrl >> (2 * (i & 3))) & 3);                                       // quad_perm
    }
    template <int CTRL, int BANKS> static Lanes sel(Lanes old, Lanes src) {
        Lanes r = old;
        for (int i = 0; i < 16; i++) if ((BANKS >> (i >> 2)) & 1) r.v[i] = src.v[source(CTRL, i)];
        return r;
    }
    template <int CTRL> static Lanes mov(Lanes v) { return sel<CTRL, 0xF>(v, v); }
    static Lanes add(Lanes a, Lanes b) {
        Lanes r;
        for (int i = 0; i < 16; i++) { volatile double s = a.v[i] + b.v[i]; r.v[i] = s; }
        return r;
    }
};
// value k of lane l of group q: sign, exponent -40 .. 40 and mantissa from splitmix64 of the element's number (tests/sp_arith_inputs.py: the same)
double group_input(uint64_t q, int nvals, int k, int l) {
    const uint64_t z = splitmix(((q * 16 + (uint64_t)nvals) * 16 + (uint64_t)k) * 16 + (uint64_t)l);
    const uint64_t e = 1023 - 40 + (z >> 1) % 81, sign = z & 1, mant = z >> 12;
    return d_of((sign << 63) | (e << 52) | mant);
}
uint64_t input_sum = 0;
long long order_matters = 0, order_cases = 0;
void check_group(uint64_t q, int nvals) {
    Lanes v[10], ref[10];
    for (int k = 0; k < nvals; k++) {
        for (int l = 0; l < 16; l++) { v[k].v[l] = group_input(q, nvals, k, l); input_sum += b_of(v[k].v[l]) * (uint64_t)(2 * l + 1); }
        ref[k] = sp_group_sum<ArrayOps>(v[k]);
        for (int l = 1; l < 16; l++)
            if (b_of(ref[k].v[l]) != b_of(ref[k].v[0])) fail("the butterfly's total differs between lanes", (double)q, k, ref[k].v[l], ref[k].v[0]);
        volatile double s = 0.0;
        for (int l = 0; l < 16; l++) s = s + v[k].v[l];
        order_cases++;
        if (b_of((double)s) != b_of(ref[k].v[0])) order_matters++;
    }
    checked++;
    if (nvals == 4) {
        const Lanes r = sp_group_sum4<ArrayOps>(v[0], v[1], v[2], v[3]);
        for (int l = 0; l < 16; l++)
            if (b_of(r.v[l]) != b_of(ref[l >> 2].v[l])) fail("group_sum4", (double)q, l, r.v[l], ref[l >> 2].v[l]);
    } else {
        const SpHessSums<Lanes> h = sp_group_sum10<ArrayOps>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
        double m[16], w[16];
        for (int i = 0; i < 16; i++) m[i] = std::numeric_limits<double>::quiet_NaN();
        for (int l = 0; l < 16; l++) sp_hessian_store(m, l, h.c0.v[l], h.c1.v[l], h.c2.v[l]);
        const double H00 = ref[0].v[0], H01 = ref[1].v[0], H02 = ref[2].v[0], H03 = ref[3].v[0], H11 = ref[4].v[0], H12 = ref[5].v[0], H13 = ref[6].v[0],
                     H22 = ref[7].v[0], H23 = ref[8].v[0], H33 = ref[9].v[0];
        // what lane 0 of the group stored from the ten butterflies
        w[0] = H00 + 5; w[1] = H01; w[2] = H02; w[3] = H03; w[4] = H01; w[5] = H11 + 5; w[6] = H12; w[7] = H13;
        w[8] = H02; w[9] = H12; w[10] = H22 + 5; w[11] = H23; w[12] = H03; w[13] = H13; w[14] = H23; w[15] = H33 + 5;
        for (int i = 0; i < 16; i++)
            if (b_of(m[i]) != b_of(w[i])) fail("group_sum10 + hessian_store", (double)q, i, m[i], w[i]);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const bool all = argc > 1 && !std::strcmp(argv[1], "--all");
    const int groups = 2048;   // (tests/sp_arith_inputs.py: GROUPS)
    // the inputs of the group sums must be sensitive to the order of the additions before they can show anything
    for (int q = 0; q < groups; q++) { check_group((uint64_t)q, 4); check_group((uint64_t)q, 10); }
    std::printf("sp_arith_host: groups checksum %016llx, a left-to-right sum differs from the butterfly in %lld of %lld sums\n", (unsigned long long)input_sum,
                order_matters, order_cases);
    if (4 * order_matters < order_cases) { std::fprintf(stderr, "the group inputs are not sensitive to the order of the additions\n"); failures++; }
    if (all) div100_all(); else div100_quick();
    std::printf("sp_arith_host: div100 %s: q0 = p * 0.01 alone is wrong for %lld floats\n", all ? "over all finite non-negative floats" : "quick set", q0_wrong);
    if (q0_wrong == 0) { std::fprintf(stderr, "q0 alone is never wrong: the div100 set shows nothing\n"); failures++; }
    cost_cases(all ? 400000000ll : 2000000ll);
    newton_cases(all ? 7u : 4099u);
    std::printf("sp_arith_host: %lld cases checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
