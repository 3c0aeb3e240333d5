// What the non-arithmetic instructions of the fast-mode KS sub-step loop cost a lone wave, by the method of
// dpp_rate.hip: one wave per SIMD (1024 waves of 64 lanes), about 10^6 instructions per wave, ns per wave-instruction;
// and the loop's own cost per trip (the taken branch and the instruction fetch behind it), which every pattern shows.
//   a. v_add_f64 on 8 independent registers against one back-to-back dependent v_add_f64 chain (the reward chain of
//      stage 1), and the chain with one independent add between its links
//   b. s_mov_b64 exec, sN / v_fma_f64 alternating, as KS_MASKED_SELECT emits them, against the same FMAs with EXEC
//      untouched (what one scalar write of EXEC costs between two FMAs)
//   c. v_cmpx_gt_f64 (the compare writes EXEC itself), followed at once by a v_fma_f64, against (b)
//   d. v_cmp_gt_f64 into an SGPR pair that an s_mov_b64 exec reads 1, 4 and 16 instructions later (how far ahead of
//      the scalar unit a mask has to be formed)
//   e. the same v_fmac_f64 with its constant in an SGPR pair (a 4-byte instruction) and as a 32-bit literal (8 bytes;
//      every VOP3 instruction above is 8 bytes too): what the instruction fetch costs a lone wave per byte of code
// Every pattern leaves EXEC as it found it.  Next to the ns stand the cycles of the shader clock (s_memtime around the
// loop of wave 0): the clock follows the power the pattern draws, the cycle count does not.
// build + run on the GPU box:  hipcc -O3 --offload-arch=gfx950 -o issue_slots tools/micro/issue_slots.hip && ./issue_slots
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

enum { ADD_INDEP, ADD_CHAIN, ADD_CHAIN_GAP1, FMA_PLAIN, FMA_SMOV_EXEC, FMA_VCMP_EXEC,
       CMP_SMOV_D1, CMP_SMOV_D4, CMP_SMOV_D16, FMAC_SGPR, FMAC_LITERAL, N_MODES };

// instructions of one block of a pattern (a trip of the loop repeats the block until it holds TRIP = 64 or 256 of them)
__host__ __device__ constexpr int per_block(int mode) {
    return mode == ADD_INDEP || mode == ADD_CHAIN || mode == FMA_PLAIN || mode == FMAC_SGPR || mode == FMAC_LITERAL ? 8
         : mode == ADD_CHAIN_GAP1 ? 16
         : mode == FMA_SMOV_EXEC || mode == FMA_VCMP_EXEC ? 16
         : mode == CMP_SMOV_D1 ? 16 : mode == CMP_SMOV_D4 ? 16 : 32;
}

#define FMA(i) "v_fma_f64 %[d" #i "], %[d" #i "], %[m], %[e]\n\t"
#define ADDI(i) "v_add_f64 %[d" #i "], %[d" #i "], %[e]\n\t"
#define FMAC_S(i) "v_fmac_f64_e32 %[d" #i "], %[sc], %[e]\n\t"
#define FMAC_L(i) "v_fmac_f64_e32 %[d" #i "], 0x3fd00000, %[e]\n\t"
#define CHAIN "v_add_f64 %[acc], %[acc], %[e]\n\t"
#define D_OUT [d0] "+v"(d[0]), [d1] "+v"(d[1]), [d2] "+v"(d[2]), [d3] "+v"(d[3]), [d4] "+v"(d[4]), [d5] "+v"(d[5]), \
              [d6] "+v"(d[6]), [d7] "+v"(d[7]), [acc] "+v"(acc)
#define D_IN [m] "v"(mul), [e] "v"(eps), [neg] "v"(neg), [ex] "s"(ex0), [ma] "s"(ma), [mb] "s"(mb), [sc] "s"(sc)

template <int MODE, int TRIP>
__global__ void __launch_bounds__(64) slot_kernel(double* out, long long* clk, int iters) {
    double d[8], acc = 0.0;
    const long long t0 = __builtin_amdgcn_s_memtime();   // shader-clock counter: the cycle figure does not depend on DVFS
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = 1.0 + 1e-9 * (threadIdx.x + i);
    const double mul = 1.0000001, eps = 1e-12, neg = -1.0 - threadIdx.x;
    const unsigned long long ex0 = __builtin_amdgcn_read_exec();
    double sc = 0.25;
    asm volatile("" : "+s"(sc));
    // two masks, both subsets of ex0, as the select's v_cmp would form them
    const unsigned long long ma = __builtin_amdgcn_fcmp(neg, -8.0, 4), mb = __builtin_amdgcn_fcmp(neg, -40.0, 4);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rep = 0; rep < TRIP / per_block(MODE); ++rep) {
            if constexpr (MODE == ADD_INDEP)
                asm volatile(ADDI(0) ADDI(1) ADDI(2) ADDI(3) ADDI(4) ADDI(5) ADDI(6) ADDI(7) : D_OUT : D_IN);
            if constexpr (MODE == ADD_CHAIN)
                asm volatile(CHAIN CHAIN CHAIN CHAIN CHAIN CHAIN CHAIN CHAIN : D_OUT : D_IN);
            if constexpr (MODE == ADD_CHAIN_GAP1)
                asm volatile(CHAIN ADDI(0) CHAIN ADDI(1) CHAIN ADDI(2) CHAIN ADDI(3) CHAIN ADDI(4) CHAIN ADDI(5) CHAIN ADDI(6)
                             CHAIN ADDI(7) : D_OUT : D_IN);
            if constexpr (MODE == FMA_PLAIN)
                asm volatile(FMA(0) FMA(1) FMA(2) FMA(3) FMA(4) FMA(5) FMA(6) FMA(7) : D_OUT : D_IN);
            if constexpr (MODE == FMAC_SGPR)
                asm volatile(FMAC_S(0) FMAC_S(1) FMAC_S(2) FMAC_S(3) FMAC_S(4) FMAC_S(5) FMAC_S(6) FMAC_S(7) : D_OUT : D_IN);
            if constexpr (MODE == FMAC_LITERAL)
                asm volatile(FMAC_L(0) FMAC_L(1) FMAC_L(2) FMAC_L(3) FMAC_L(4) FMAC_L(5) FMAC_L(6) FMAC_L(7) : D_OUT : D_IN);
            if constexpr (MODE == FMA_SMOV_EXEC)
                asm volatile("s_mov_b64 exec, %[ma]\n\t" FMA(0) "s_mov_b64 exec, %[mb]\n\t" FMA(1)
                             "s_mov_b64 exec, %[ma]\n\t" FMA(2) "s_mov_b64 exec, %[mb]\n\t" FMA(3)
                             "s_mov_b64 exec, %[ma]\n\t" FMA(4) "s_mov_b64 exec, %[mb]\n\t" FMA(5)
                             "s_mov_b64 exec, %[ma]\n\t" FMA(6) "s_mov_b64 exec, %[ex]\n\t" FMA(7) : D_OUT : D_IN);
            if constexpr (MODE == FMA_VCMP_EXEC)
                // every compare runs with EXEC = ex0 only in the first place; afterwards with the mask it wrote itself,
                // which the compare reproduces (neg < 0 in every lane); the last write restores ex0
                asm volatile("v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(0) "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(1)
                             "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(2) "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(3)
                             "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(4) "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(5)
                             "v_cmpx_gt_f64_e32 vcc, 0, %[neg]\n\t" FMA(6) "s_mov_b64 exec, %[ex]\n\t" FMA(7)
                             : D_OUT : D_IN : "vcc");
            if constexpr (MODE == CMP_SMOV_D1)
                // v_cmp -> SGPR pair -> s_mov_b64 exec right behind it, then 6 FMAs: 8 instructions, twice
                asm volatile("v_cmp_gt_f64_e64 s[50:51], 0, %[neg]\n\ts_mov_b64 exec, s[50:51]\n\t" FMA(0) FMA(1) FMA(2)
                             "s_mov_b64 exec, %[ex]\n\t" FMA(3) FMA(4)
                             "v_cmp_gt_f64_e64 s[50:51], 0, %[neg]\n\ts_mov_b64 exec, s[50:51]\n\t" FMA(5) FMA(6) FMA(7)
                             "s_mov_b64 exec, %[ex]\n\t" FMA(0) FMA(1) : D_OUT : D_IN : "s50", "s51");
            if constexpr (MODE == CMP_SMOV_D4)
                asm volatile("v_cmp_gt_f64_e64 s[50:51], 0, %[neg]\n\t" FMA(0) FMA(1) FMA(2) "s_mov_b64 exec, s[50:51]\n\t"
                             "s_mov_b64 exec, %[ex]\n\t" FMA(3) FMA(4)
                             "v_cmp_gt_f64_e64 s[50:51], 0, %[neg]\n\t" FMA(5) FMA(6) FMA(7) "s_mov_b64 exec, s[50:51]\n\t"
                             "s_mov_b64 exec, %[ex]\n\t" FMA(0) FMA(1) : D_OUT : D_IN : "s50", "s51");
            if constexpr (MODE == CMP_SMOV_D16)
                asm volatile("v_cmp_gt_f64_e64 s[50:51], 0, %[neg]\n\t" FMA(0) FMA(1) FMA(2) FMA(3) FMA(4) FMA(5) FMA(6) FMA(7)
                             FMA(0) FMA(1) FMA(2) FMA(3) FMA(4) FMA(5) FMA(6) "s_mov_b64 exec, s[50:51]\n\t"
                             "s_mov_b64 exec, %[ex]\n\t" FMA(7) FMA(0) FMA(1) FMA(2) FMA(3) FMA(4) FMA(5) FMA(6) FMA(7)
                             FMA(0) FMA(1) FMA(2) FMA(3) FMA(4) : D_OUT : D_IN : "s50", "s51");
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
    double s = acc;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += d[i];
    if (s == 12345.678) out[0] = s;
}

template <int MODE, int TRIP>
double trip_cycles(double* d_out, float* ms) {
    const int iters = (1 << 20) / TRIP, waves = 1024;     // 1 wave per SIMD on 256 CUs, 2^20 instructions per wave
    long long* clk = (long long*)(d_out + 1);
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    hipLaunchKernelGGL((slot_kernel<MODE, TRIP>), dim3(waves), dim3(64), 0, 0, d_out, clk, 100);
    (void)hipEventRecord(a);
    hipLaunchKernelGGL((slot_kernel<MODE, TRIP>), dim3(waves), dim3(64), 0, 0, d_out, clk, iters);
    (void)hipEventRecord(b);
    (void)hipEventSynchronize(b);
    (void)hipEventElapsedTime(ms, a, b);
    long long cycles = 0;
    (void)hipMemcpy(&cycles, clk, 8, hipMemcpyDeviceToHost);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return (double)cycles / iters;
}

// A trip of 64 and a trip of 256 instructions differ by 192 instructions and not by the loop's own cost (counter,
// compare, taken branch and the instruction fetch behind it): the difference gives the cycles per instruction, the
// rest of the short trip the cost of going round the loop once.
template <int MODE>
void run(const char* name, int group) {
    static double* d_out = nullptr;
    if (!d_out && hipMalloc(&d_out, 16) != hipSuccess) exit(1);
    float ms64 = 0, ms256 = 0;
    const double c64 = trip_cycles<MODE, 64>(d_out, &ms64), c256 = trip_cycles<MODE, 256>(d_out, &ms256);
    const double per = (c256 - c64) / 192.0;
    printf("%-60s %7.3f ns/instr (%.2f GHz)  trips of 64 / 256: %7.1f / %7.1f cycles  -> %6.3f cycles per instruction, "
           "%5.1f per group of %d, loop %5.1f cycles per trip\n", name, ms256 * 1e6 / (1 << 20),
           c256 * ((1 << 20) / 256) / (ms256 * 1e6), c64, c256, per, per * group, group, c64 - 64 * per);
}

int main() {
    for (int pass = 0; pass < 2; ++pass) {
        printf("pass %d\n", pass);
        run<ADD_INDEP>("a  v_add_f64, 8 independent registers", 1);
        run<ADD_CHAIN>("a  v_add_f64, one dependent chain", 1);
        run<ADD_CHAIN_GAP1>("a  chain link + 1 independent add", 2);
        run<FMA_PLAIN>("b  v_fma_f64, EXEC untouched", 1);
        run<FMA_SMOV_EXEC>("b  (s_mov_b64 exec, sN; v_fma_f64) x 8", 2);
        run<FMA_VCMP_EXEC>("c  (v_cmpx_gt_f64; v_fma_f64) x 7 + (s_mov exec; v_fma_f64)", 16);
        run<CMP_SMOV_D1>("d  v_cmp -> s_mov exec next; 2 s_mov + 1 v_cmp + 5 fma", 8);
        run<CMP_SMOV_D4>("d  v_cmp -> s_mov exec 4 later; same 8 instructions", 8);
        run<CMP_SMOV_D16>("d  v_cmp -> s_mov exec 16 later; 2 s_mov + 1 v_cmp + 29 fma", 32);
        run<FMAC_SGPR>("e  v_fmac_f64_e32 v, s, v: constant in an SGPR pair (4 bytes)", 1);
        run<FMAC_LITERAL>("e  v_fmac_f64_e32 v, literal, v: the same constant (8 bytes)", 1);
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
