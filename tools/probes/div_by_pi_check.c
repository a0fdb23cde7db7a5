// div_by_pi_check.c -- does saturate(x) / pi survive the product-and-remainder form that replaces (float)byte / 255 (byte_over_255,
// voxel_rt2_amd/csrc/vrt_types.h)?  Every one of the 2^32 patterns of x goes through saturate() as the device evaluates it (a NaN
// operand of min / max is ignored) and both forms; the forms are compared by their bits.
//     gcc -O2 -fopenmp -mfma -ffp-contract=off -fno-fast-math tools/probes/div_by_pi_check.c -o div_by_pi_check && ./div_by_pi_check
// Answer (x86-64, about half a minute): 1 481 822 patterns differ, 1 229 056 of them with a normal numerator (pi's reciprocal is not
// a byte's: one correction step does not always land on the rounded quotient) and the rest subnormal -- so pdf_diffuse_lobe() and its
// kin keep their division (a guarded form was measured slower before: profiles/README.md).
#include <stdio.h>
#include <stdint.h>
#include <string.h>
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
#define PI 3.14159274101257324f
static inline float vmax(float a, float b) { if (a != a) return b; if (b != b) return a; return a > b ? a : b; }
static inline float vmin(float a, float b) { if (a != a) return b; if (b != b) return a; return a < b ? a : b; }
static inline int differs(float s, float r) {
    volatile float den = PI;   // (no reciprocal substituted by the compiler)
    const float want = s / den;
    const float q0 = s * r, rem = __builtin_fmaf(-q0, PI, s), got = __builtin_fmaf(rem, r, q0);
    return f2u(want) != f2u(got);
}
int main(void) {
    const float r = 1.0f / PI;
    unsigned long long bad = 0, bad_normal = 0;
#pragma omp parallel for reduction(+ : bad, bad_normal) schedule(static)
    for (long long i = 0; i < (1LL << 32); i++) {
        const float s = vmin(vmax(u2f((uint32_t)i), 0.0f), 1.0f);
        if (differs(s, r)) { bad++; if (s >= 1.17549435e-38f) bad_normal++; }
    }
    printf("patterns that differ: %llu of 2^32, %llu of them with a normal numerator\n", bad, bad_normal);
    return bad != 0;
}
