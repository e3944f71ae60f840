// Micro-benchmark, sibling of fetch_rate.hip: what do the issue slots that compute nothing cost ONE lone wavefront on an idle CU of gfx950
// (the 4096-env regime of the persistent rollout kernel: one physics wave per SIMD)?
//   hipcc -O3 --offload-arch=gfx950 -o slot_cost tools/micro/slot_cost.hip && ./slot_cost
// Each body element is the instruction group named below, repeated UNROLL x 4 times per loop pass (on 4 independent chains or on 1),
// in inline asm so that the compiler neither folds, packs nor reorders.  Printed: cycles per ELEMENT, and per element beyond case (a).
//   (a) v_pk_fma_f32 with a resident SGPR-pair splat operand (op_sel_hi:[1,0,1]: both halves read the low register)
//   (b) the same, preceded each time by s_mov_b32 of a fresh literal into that SGPR       -- a re-materialised model constant
//   (c) (a) preceded by a v_mov_b32 into the low half of a VGPR pair the v_pk_fma reads   -- the zero half of a pair
//   (d) v_mul_f32 and v_fmac_f32 with a 32-bit literal (the scalar form's free constants), one element = the two instructions
//   (e) two v_fma_f32 on VGPRs                                                            -- what a v_pk_fma_f32 replaces
// The fixed registers s[20:21] and v[30:31] are declared as clobbers; nothing but out[0..63] and *cyc is written to memory.
#include <hip/hip_runtime.h>
#include <cstdio>

typedef float f2 __attribute__((ext_vector_type(2)));

// one asm statement holds four elements (chains 0..3, or chain 0 four times when CH == 1), so that whatever the compiler puts between two
// statements (it pads some register re-uses across statements with s_nop 0) is the same in every case: one group per four elements
#define SLOT4(TEXT, ...) \
    if (CH == 1) asm volatile(TEXT(0, 4) TEXT(0, 5) TEXT(0, 6) TEXT(0, 7) : "+v"(P0), "+v"(P1), "+v"(P2), "+v"(P3) : __VA_ARGS__); \
    else asm volatile(TEXT(0, 4) TEXT(1, 5) TEXT(2, 6) TEXT(3, 7) : "+v"(P0), "+v"(P1), "+v"(P2), "+v"(P3) : __VA_ARGS__);
#define LIT4 "i"(0x3f800001 + 4*u), "i"(0x3f800002 + 4*u), "i"(0x3f800003 + 4*u), "i"(0x3f800004 + 4*u)
#define T_A(k, l) "v_pk_fma_f32 %" #k ", %8, %9, %" #k " op_sel_hi:[1,0,1]\n\t"
#define T_B(k, l) "s_mov_b32 s20, %" #l "\n\tv_pk_fma_f32 %" #k ", %8, s[20:21], %" #k " op_sel_hi:[1,0,1]\n\t"
#define T_C(k, l) "v_mov_b32 v30, %9\n\tv_pk_fma_f32 %" #k ", %8, v[30:31], %" #k "\n\t"
#define T_D(k, l) "v_mul_f32_e32 %" #k ", 0x3f800001, %" #k "\n\tv_fmac_f32_e32 %" #k ", 0x33d6bf95, %8\n\t"
#define T_E(k, l) "v_fma_f32 %" #k ", %8, %8, %" #k "\n\tv_fma_f32 %" #k ", %8, %8, %" #k "\n\t"

template <int UNROLL, int KIND, int CH>
__global__ void __launch_bounds__(64) body(float* out, int iters, long long* cyc) {
    const int lane = threadIdx.x;
    const float y = 1e-7f*(1 + lane);
    float x0 = 1.0f + lane*1e-3f, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3;
    f2 p0 = f2{x0, x0 + 1.0f}, p1 = p0 + 1.0f, p2 = p0 + 2.0f, p3 = p0 + 3.0f;
    const f2 py = f2{y, y};
    const unsigned long long splat = 0x3f8000013f800001ull;          // (1 + ulp, 1 + ulp): loop-invariant, so it stays in an SGPR pair
    asm volatile("s_mov_b32 s20, 0x3f800001\n\ts_mov_b32 s21, 0x3f800001\n\tv_mov_b32 v30, 0\n\tv_mov_b32 v31, 0" ::: "s20", "s21", "v30", "v31");
    const long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
#define P0 p0
#define P1 p1
#define P2 p2
#define P3 p3
            if (KIND == 0) { SLOT4(T_A, LIT4, "v"(py), "s"(splat)) }
            if (KIND == 1) { SLOT4(T_B, LIT4, "v"(py) : "s20") }
            if (KIND == 2) { SLOT4(T_C, LIT4, "v"(py), "v"(y) : "v30") }
#undef P0
#undef P1
#undef P2
#undef P3
#define P0 x0
#define P1 x1
#define P2 x2
#define P3 x3
            if (KIND == 3) { SLOT4(T_D, LIT4, "v"(y)) }
            if (KIND == 4) { SLOT4(T_E, LIT4, "v"(y)) }
#undef P0
#undef P1
#undef P2
#undef P3
        }
    }
    const long long t1 = __builtin_readcyclecounter();
    out[lane] = x0 + x1 + x2 + x3 + p0.x + p0.y + p1.x + p1.y + p2.x + p2.y + p3.x + p3.y;
    if (lane == 0) *cyc = t1 - t0;
}

template <int UNROLL, int KIND, int CH> double run(float* out, long long* cyc, const char* name, double base) {
    const int iters = 65536/UNROLL/4; long long c = 0;
    for (int rep = 0; rep < 3; rep++) {
        hipLaunchKernelGGL((body<UNROLL, KIND, CH>), dim3(1), dim3(64), 0, 0, out, iters, cyc);
        if (hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("hipMemcpy failed\n"); exit(1); }
    }
    const double per = c/((double)iters*UNROLL*4);
    printf("%-58s chains %d  body %4d elements: %6.2f cycles / element", name, CH, UNROLL*4, per);
    if (base > 0) printf("   (%+.2f beyond (a))", per - base);
    printf("\n");
    return per;
}

template <int CH> void all(float* out, long long* cyc) {
    const double a = run<64, 0, CH>(out, cyc, "(a) v_pk_fma_f32, resident SGPR-pair splat", 0);
    run<64, 1, CH>(out, cyc, "(b) s_mov_b32 literal + v_pk_fma_f32", a);
    run<64, 2, CH>(out, cyc, "(c) v_mov_b32 into a pair half + v_pk_fma_f32", a);
    run<64, 3, CH>(out, cyc, "(d) v_mul_f32 literal + v_fmac_f32 literal", a);
    run<64, 4, CH>(out, cyc, "(e) v_fma_f32 + v_fma_f32", a);
}

int main() {
    float* out; long long* cyc;
    if (hipMalloc(&out, 256) != hipSuccess || hipMalloc(&cyc, 8) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    all<1>(out, cyc); all<4>(out, cyc);
    return 0;
}
